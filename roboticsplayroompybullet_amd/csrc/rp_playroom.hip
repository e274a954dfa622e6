/* rp_playroom.hip — C ABI (include/rp_playroom.h) over the gfx950 kernels in rp_kernels.cuh. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/rp_playroom.h"
#include "../../include/rp_playroom_debug.h"
#include "generated/rp_models_gen.h"
#include "generated/rp_hullverts_gen.h"
#include "generated/rp_hullcells_gen.h"
#include "generated/rp_hullplanes_gen.h"
#include "rp_device_model.h"
#include "rp_kernels.cuh"
#include "rp_render.cuh"
#include "rp_closest.cuh"


/* a by-value kernel argument (k_render_views' table) and the host's one record of a view: its layout must not move */
static_assert(sizeof(RpViewEntry) == 128, "RpViewEntry is a by-value kernel argument: its layout must not move");

/* THE image configuration of a handle (image_config_set; n = 0: none): k_render_views' table of the observation pass and that of the terminal pass - the views with a
 * final_* pointer, with those pointers, n_fin of them -, each with its tile count, and the clouds attached to the views (rp_set_image_points: pc_n = how many views
 * have one; pc_obs[k] / pc_fin[k] are view k's entries for the two passes, pc_has[k] bit 0 / bit 1 = which exist; dropped with the configuration) */
struct RpImageConfig {
  int n, n_fin, tiles, ftiles;
  RpViewTable obs, fin;
  int fmap[RC_MAX_VIEWS];         /* view -> its entry of fin, -1: the view has no terminal layers */
  int pc_n, pc_has[RC_MAX_VIEWS]; RpPointsEntry pc_obs[RC_MAX_VIEWS], pc_fin[RC_MAX_VIEWS];
};

struct rp_sim {
  rp_config cfg;
  DevModel host_model;
  DevModel* dev_model;
  float* state;            /* [N][RP_REC_FLOATS] */
  float* ws;               /* [N][W3_FLOATS] constraint-row workspace of the split step pipeline */
  float* dbg;
  float* hullv;            /* convex-hull vertices of the arm's collision meshes (DevModel.hullv points here) */
  float* hcv; int* hco;    /* their support-vertex candidate tables (DevModel.hcv / hco) */
  float* hpl;              /* their face planes, collider frame (DevModel.hpl: the ray caster) */
  float* pmcache;          /* the contact caches, [N][PMC_FLOATS] (DevModel.pmcache points here); nullptr under RP_CFG_STATELESS_CONTACTS */
  float* dyn;              /* the per-env dynamics table, [N][n_obj + n_free] (DevModel.dyn points here) */
  float* wrench;           /* the per-env wrench table, [N][n_arm + n_free + n_j1][6] (DevModel.wrench points here) */
  float* act;              /* the per-env actuation table, [N][3 + 2 n_arm]: gravity, motor gains, motor strengths (DevModel.act points here) */
  int* sort_cnt;           /* [2][RP_MAX_GROUPS][SORT_BINS] load-class histograms for pairing envs in k_solve2 (double-buffered) */
  int* sort_slot;          /* [N] per env: (bin << 16) | rank inside the bin, from the latest k_solve2 */
  int* pair_env;           /* [N] per group range: env ids sorted by load class, heaviest first (k_solve2 pairs neighbours) */
  int* hv_list;            /* [N] per group range: the heavy envs of the current substep (k_prep2 appends, k_solve2's worker blocks take them: one env per wave) */
  int hv_waves;            /* worker blocks per group (0: an eighth of the group's envs, 16 .. 512; RP_HV_WAVES overrides) */
  int* hv_cnt;             /* [2][RP_MAX_GROUPS] their number, double-buffered by substep parity (zeroed by k_member and by the k_prep2 before) */
  GroupBounds gb;          /* place ranges of the groups the tables were built for */
  int gsplit[RP_MAX_GROUPS]; /* RP_GROUP_SPLIT: relative sizes of the groups, heaviest first (0 = equal) */
  int* member[2];          /* [N] place -> env, all envs ranked by load class (k_member); group g owns places [N g / G, N (g + 1) / G) */
  int member_cur;
  int debug_flags;         /* rp_set_debug_flags: bit 0 = k_solve2 never solves contacts side by side (one folded slot per contact) */
  int sort_G, sort_par;    /* group count the tables were built for (0 = none yet); buffer that the next k_solve2 reads */
  hipEvent_t ev0, ev1;
  hipEvent_t* pool;        /* per-launch timing ring: EV_PER_STEP events per recorded step */
  int pool_steps, pool_next, pool_count;
  int timers_on;
  int groups;              /* env groups of the default pipeline, each on its own stream (tail overlap) */
  hipStream_t gstream[RP_MAX_GROUPS];
  hipEvent_t gfork, gjoin[RP_MAX_GROUPS];
  int fused;               /* 0: split pipeline (default), 1: single fused k_step kernel (in-library reference path), 2: k_chain - one launch for the twelve substeps (round 4's experiment) */
  int chain_blocks;        /* k_chain's grid (RP_CHAIN_BLOCKS at rp_create, default 1024) */
  /* rp_reset through the split pipeline (allocated at the first reset): dense scratch records of the envs that are settling,
   * their env ids, per-env progress {pending, attempt, depth}, pairing tables of the scratch range */
  float* rs_state; int* rs_idx; int4* rs_meta; int* rs_count; int* rs_sort_cnt; int* rs_sort_slot; int* rs_pair; int* rs_count_host;
  int reset_rounds;        /* rounds the latest rp_reset took (rp_debug) */
  float* rc_tab; int* rc_cnt; float* rc_ee; int rc_cap; int rc_last_num;      /* rp_render / rp_ray_test: collider poses of rc_cap envs (allocated on first use) */
  int render_nocull;       /* rp_debug_render_cull(h, 0): k_render_layers lists every record for every tile (rp_render, rp_render_ex, rp_render_layers) */
  int rs_chunk;            /* rp_debug_render_states_chunk(h, slots): rp_render_states' chunks hold at most this many images (0: max(N, 4096)) */
  /* rp_step_autoreset: episode counters [N], the list of ending envs [N], its length and take counter [2], k_autoreset's pairing table [4 * ar_grid] */
  int* ep_steps; int* ar_list; int* ar_ctl; int* ar_pair;
  int ar_grid, ar_epb;     /* k_autoreset's grid (the blocks resident at once; RP_AUTORESET_BLOCKS overrides) and envs per block (RP_AUTORESET_EPB, 1 .. 4, default 1) */
  int32_t ar_max_steps; uint32_t ar_when;      /* rp_set_autoreset */
  float* cp_stage;         /* rp_copy_envs: one staged copy of every state row, [N][RP_REC_FLOATS + (PMC_FLOATS)], and behind it the episode counters [N] (allocated at the first call) */
  float* vis;              /* rp_set_visuals / rp_get_visuals: the per-env visuals table, [N][3 n_col + VIS_TAIL] = colour[n_col][3] light[5] background[3], and behind it the default
                            * light and background (allocated and filled at the first call; nullptr until then: the render kernels take the baked colours and their literals) */
  /* rp_set_reset_table: the table [rt_rows, rt_n_o] (rt_rows = 0: none), the row cursor [1], each env's row of the latest autoreset step [N] (-1: none), the waves' ballots
   * and first rows [(N + 255) / 256 * 4]; k_autoreset_to's grid (the waves resident at once) */
  float* rt_tab; int rt_rows, rt_n_o; int* rt_cursor; int* rt_env_row; unsigned long long* rt_wave_bal; int* rt_wave_row; int rt_grid;
  rp_timers timers;
  char err[256];
  int iv_nomerge;          /* rp_debug_image_views_merge(h, 0): a k_render_layers launch per view instead of one k_render_views */
  RpImageConfig img;       /* rp_set_image_obs / rp_set_image_views / rp_set_image_points (behind everything else: the kilobytes of tables stand among no other fields) */
};

#define EV_PER_STEP (2 + 2 * (2 * K_NSUB + 2))   /* step pair + a pair per launch (action, 12 prep, 12 solve, obs) */
static thread_local char g_err[256] = "";   /* rp_create / NULL-handle errors: per calling thread (rp_last_error(NULL) reads the caller's own) */

#define HIPCHK(h, call)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (call);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      snprintf((h) ? (h)->err : g_err, 256, "%s failed: %s", #call, hipGetErrorString(e_));         \
      return RP_ERR_HIP;                                                                            \
    }                                                                                               \
  } while (0)

/* makes the handle's device current for one entry point and restores the caller's on the way out (handles on several devices,
 * or a torch caller whose current device is another one) */
struct DevGuard {
  int prev = -1, cur = -1;
  explicit DevGuard(int dev) : cur(dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != cur) (void)hipSetDevice(cur);
  }
  ~DevGuard() { if (prev >= 0 && prev != cur) (void)hipSetDevice(prev); }
};

/* the one path of the per-env parameter tables (dynamics, wrench, actuation; k_set_table / k_get_table): rows_ok is the `rows` check every set entry point makes,
 * launch_table_set the bare launch over table [num_envs][c.w0 + c.w1 + c.w2] (rp_create fills its default rows with it), table_set / table_get an entry point's
 * checked launch on `stream` */
static bool rows_ok(rp_sim* h, const char* fn, int32_t rows) {
  if (rows == 1 || rows == h->cfg.num_envs) return true;
  snprintf(h->err, 256, "%s: rows = %d, expected 1 or num_envs = %d", fn, rows, h->cfg.num_envs);
  return false;
}
static void launch_table_set(rp_sim* h, float* tab, TabCols<const float> c, int null_is_zero, int rows, const uint8_t* mask, void* stream) {
  const int N = h->cfg.num_envs;
  const size_t total = (size_t)N * (c.w0 + c.w1 + c.w2);
  hipLaunchKernelGGL(k_set_table, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, c, null_is_zero, rows, mask, N);
}
static int table_set(rp_sim* h, const char* fn, float* tab, TabCols<const float> c, int null_is_zero, int32_t rows, const uint8_t* mask, void* stream) {
  if (!rows_ok(h, fn, rows)) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  launch_table_set(h, tab, c, null_is_zero, (int)rows, mask, stream);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}
static int table_get(rp_sim* h, const float* tab, TabCols<float> c, void* stream) {
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs;
  const size_t total = (size_t)N * (c.w0 + c.w1 + c.w2);
  hipLaunchKernelGGL(k_get_table, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tab, c, N);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

static void image_pass(rp_sim* h, bool final, const int32_t* sel32, const uint8_t* sel8, hipStream_t s);      /* (beside the render entry points, below) */
static void points_pass(rp_sim* h, bool final, const int32_t* sel32, const uint8_t* sel8, hipStream_t s);

static OutPtrs to_ptrs(const rp_out* o) {
  OutPtrs p;
  memset(&p, 0, sizeof(p));
  if (!o) return p;
  p.obs_quat = o->obs_quat; p.achieved_goal = o->achieved_goal; p.desired_goal = o->desired_goal;
  p.cag = o->controllable_achieved_goal; p.fps = o->full_positional_state; p.joints = o->joints; p.velocity = o->velocity;
  p.observation = o->observation; p.proprio = o->gripper_proprioception; p.reward = o->reward; p.is_success = o->is_success;
  p.target_poses = o->target_poses; p.status = o->status; p.pack = o->pack;
  return p;
}

extern "C" {

#ifndef RP_BUILD_ID
#define RP_BUILD_ID "unversioned"
#endif
#ifdef RP_WIDE
const char* rp_version(void) { return "rp_playroom 0.5.2 (gfx950, wide build: two-object play ids) build " RP_BUILD_ID; }
#else
const char* rp_version(void) { return "rp_playroom 0.5.2 (gfx950) build " RP_BUILD_ID; }
#endif

static void destroy_handle(rp_sim* h) {        /* frees whatever a (possibly partial) handle owns; hipFree(nullptr) etc. are no-ops */
  if (!h) return;
  hipFree(h->hullv); hipFree(h->hcv); hipFree(h->hco); hipFree(h->hpl); hipFree(h->pmcache); hipFree(h->dyn); hipFree(h->wrench); hipFree(h->act); hipFree(h->dev_model); hipFree(h->state); hipFree(h->ws); hipFree(h->dbg); hipFree(h->sort_cnt); hipFree(h->sort_slot); hipFree(h->pair_env); hipFree(h->hv_list); hipFree(h->hv_cnt); hipFree(h->member[0]); hipFree(h->member[1]);
  hipFree(h->rc_tab); hipFree(h->rc_cnt); hipFree(h->rc_ee);
  hipFree(h->ep_steps); hipFree(h->ar_list); hipFree(h->ar_ctl); hipFree(h->ar_pair); hipFree(h->cp_stage); hipFree(h->vis);
  hipFree(h->rt_tab); hipFree(h->rt_cursor); hipFree(h->rt_env_row); hipFree(h->rt_wave_bal); hipFree(h->rt_wave_row);
  hipFree(h->rs_state); hipFree(h->rs_idx); hipFree(h->rs_meta); hipFree(h->rs_count); hipFree(h->rs_sort_cnt); hipFree(h->rs_sort_slot); hipFree(h->rs_pair);
  if (h->rs_count_host) hipHostFree(h->rs_count_host);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->gfork) hipEventDestroy(h->gfork);
  for (int i = 0; i < RP_MAX_GROUPS; i++) { if (h->gstream[i]) hipStreamDestroy(h->gstream[i]); if (h->gjoin[i]) hipEventDestroy(h->gjoin[i]); }
  if (h->pool) { for (int i = 0; i < h->pool_steps * EV_PER_STEP; i++) if (h->pool[i]) hipEventDestroy(h->pool[i]); free(h->pool); }
  free(h);
}

int rp_create(const rp_config* cfg, rp_handle* out) {
  if (!cfg || !out || cfg->num_envs <= 0) { snprintf(g_err, 256, "rp_create: bad argument"); return RP_ERR_ARG; }
  if (cfg->num_envs > RP_MAX_ENVS) { snprintf(g_err, 256, "rp_create: num_envs %d exceeds %d (rank field of the env pairing tables)", cfg->num_envs, RP_MAX_ENVS); return RP_ERR_ARG; }
  if (cfg->env_kind < 0 || cfg->env_kind >= RP_ENV_COUNT) { snprintf(g_err, 256, "rp_create: unsupported env kind %d", cfg->env_kind); return RP_ERR_UNSUPPORTED; }
  if ((cfg->flags & RP_CFG_ACTION_TYPE) && (cfg->action_type < 0 || cfg->action_type > RP_ACTION_RELATIVE_JOINTS)) { snprintf(g_err, 256, "rp_create: action_type %d", cfg->action_type); return RP_ERR_ARG; }
  if ((cfg->flags & RP_CFG_HULL_EPA) && (cfg->flags & RP_CFG_NO_HULL_EPA)) { snprintf(g_err, 256, "rp_create: RP_CFG_HULL_EPA and RP_CFG_NO_HULL_EPA"); return RP_ERR_ARG; }
  if ((cfg->flags & RP_CFG_CONTACT_MARGIN) && !(cfg->contact_margin >= 0.f && cfg->contact_margin <= 0.05f)) { snprintf(g_err, 256, "rp_create: contact_margin %g outside [0, 0.05]", (double)cfg->contact_margin); return RP_ERR_ARG; }
  /* registered id -> baked model (arm + scene) and action type.  The ids of a play family share scene, arm and configuration
   * (envList.py:43-140); only perform_action differs. */
  static const struct { char model; int action_type; } SPEC[RP_ENV_COUNT] = {
    {'U', RP_ACT_ABS_RPY}, {'R', RP_ACT_ABS_RPY}, {'P', RP_ACT_ABS_RPY},
    {'U', RP_ACT_ABS_QUAT}, {'U', RP_ACT_REL_QUAT}, {'U', RP_ACT_REL_JOINTS}, {'U', RP_ACT_ABS_JOINTS}, {'U', RP_ACT_REL_RPY},
    {'P', RP_ACT_ABS_RPY},
    {'Q', RP_ACT_ABS_RPY}, {'Q', RP_ACT_ABS_RPY},
    {'V', RP_ACT_ABS_QUAT}, {'V', RP_ACT_REL_QUAT}, {'V', RP_ACT_REL_JOINTS}, {'V', RP_ACT_ABS_JOINTS}, {'V', RP_ACT_ABS_RPY}, {'V', RP_ACT_REL_RPY},
    {'W', RP_ACT_ABS_QUAT}, {'W', RP_ACT_REL_JOINTS}};
  static_assert(RP_ACT_ABS_RPY == RP_ACTION_ABSOLUTE_RPY && RP_ACT_REL_RPY == RP_ACTION_RELATIVE_RPY && RP_ACT_ABS_QUAT == RP_ACTION_ABSOLUTE_QUAT &&
                RP_ACT_REL_QUAT == RP_ACTION_RELATIVE_QUAT && RP_ACT_ABS_JOINTS == RP_ACTION_ABSOLUTE_JOINTS && RP_ACT_REL_JOINTS == RP_ACTION_RELATIVE_JOINTS,
                "public rp_action_type values are the kernels' RP_ACT_*");
  const int action_type = (cfg->flags & RP_CFG_ACTION_TYPE) ? cfg->action_type : SPEC[cfg->env_kind].action_type;
#ifdef RP_WIDE
  if (SPEC[cfg->env_kind].model != 'W') { snprintf(g_err, 256, "rp_create: env kind %d is served by librp_playroom_hip.so, not by the wide build", cfg->env_kind); return RP_ERR_UNSUPPORTED; }
#else
  if (SPEC[cfg->env_kind].model == 'W') { snprintf(g_err, 256, "rp_create: the two-object ids (env kind %d) are served by librp_playroom_hip_wide.so", cfg->env_kind); return RP_ERR_UNSUPPORTED; }
#endif
  {
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess) { (void)hipGetLastError(); snprintf(g_err, 256, "rp_create: hipGetDeviceCount: %s", hipGetErrorString(de)); return RP_ERR_HIP; }
    if (cfg->device < 0 || cfg->device >= ndev) { snprintf(g_err, 256, "rp_create: device %d of %d", cfg->device, ndev); return RP_ERR_ARG; }
  }
  rp_sim* h = (rp_sim*)calloc(1, sizeof(rp_sim));
  rp_model* m = (rp_model*)malloc(sizeof(rp_model));
  if (!h || !m) { free(h); free(m); snprintf(g_err, 256, "rp_create: out of host memory"); return RP_ERR_ARG; }
  h->cfg = *cfg;
  switch (SPEC[cfg->env_kind].model) {
    case 'W': rp_fill_model_W(m); break;
    case 'R': rp_fill_model_R(m); break;
    case 'P': rp_fill_model_P(m); break;
    case 'Q': rp_fill_model_Q(m); break;
    case 'V': rp_fill_model_V(m); break;
    default: rp_fill_model_U(m); break;
  }
  rp_build_dev_model(m, &h->host_model);
  free(m);
  DevModel* d = &h->host_model;
  if (cfg->env_kind == RP_ENV_PANDA_PUSH) {      /* pandaPick's arm and scene with pandaPush's ranges (envList.py:12-16) */
    const float gl[3] = {-0.1f, -0.1f, -0.06f}, gh[3] = {0.1f, 0.1f, -0.05f}, eh[3] = {0.18f, 0.18f, -0.04f};
    for (int k = 0; k < 3; k++) { d->goal_lo[k] = d->obj_lo[k] = gl[k]; d->goal_hi[k] = d->obj_hi[k] = gh[k]; d->env_hi[k] = eh[k]; }
  }
  if (cfg->env_kind == RP_ENV_PANDA_REACH_2D) {  /* envList.py:24-26 */
    const float gl[3] = {-0.18f, -0.18f, -0.06f}, gh[3] = {0.18f, 0.18f, -0.05f}, eh[3] = {0.18f, 0.18f, 0.0f};
    for (int k = 0; k < 3; k++) { d->goal_lo[k] = gl[k]; d->goal_hi[k] = gh[k]; d->env_hi[k] = eh[k]; }
  }
  /* the constructor kwargs of the env class (rp_config.flags; environments.py:64-67) */
  for (int k = 0; k < 3; k++) {
    if (cfg->flags & RP_CFG_GOAL_RANGE) { d->goal_lo[k] = cfg->goal_range_low[k]; d->goal_hi[k] = cfg->goal_range_high[k]; }
    if (cfg->flags & RP_CFG_OBJ_RANGE) { d->obj_lo[k] = cfg->obj_lower_bound[k]; d->obj_hi[k] = cfg->obj_upper_bound[k]; }
    if (cfg->flags & RP_CFG_ENV_RANGE) d->env_hi[k] = cfg->env_range_high[k];
  }
  if (cfg->flags & RP_CFG_REW_THRESH) d->rew_thresh = cfg->sparse_rew_thresh;
  if (cfg->flags & RP_CFG_DENSE_REWARD) d->dense_reward = 1;
  if (cfg->flags & RP_CFG_CONTACT_MARGIN) { for (int c = 0; c < RP_MAX_COL; c++) d->col_margin[c] = cfg->contact_margin; d->boxbox_margin = -1.f; }
  d->action_type = action_type;
  d->n_action = (action_type == RP_ACT_ABS_QUAT || action_type == RP_ACT_REL_QUAT) ? 8
              : ((action_type == RP_ACT_ABS_JOINTS || action_type == RP_ACT_REL_JOINTS) ? d->n_target + 1 : 7);
  DevGuard guard(cfg->device);
  const int N = cfg->num_envs;
  int rc = RP_ERR_HIP;
  hipError_t e = hipSuccess;
#define CREATE_CHK(call) do { e = (call); if (e != hipSuccess) { snprintf(g_err, 256, "rp_create: %s: %s", #call, hipGetErrorString(e)); goto fail; } } while (0)
  (void)hipGetLastError();          /* a stale error of an earlier, unrelated call must not fail this one */
  CREATE_CHK(hipSetDevice(cfg->device));
  CREATE_CHK(hipMalloc((void**)&h->dev_model, sizeof(DevModel)));
  CREATE_CHK(hipMalloc((void**)&h->state, (size_t)N * RP_REC_FLOATS * sizeof(float)));
  CREATE_CHK(hipMalloc((void**)&h->ws, (size_t)N * W3_FLOATS * sizeof(float)));
  CREATE_CHK(hipMalloc((void**)&h->dbg, 4096 * sizeof(float)));
  CREATE_CHK(hipMalloc((void**)&h->sort_cnt, (size_t)2 * RP_MAX_GROUPS * SORT_BINS * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&h->sort_slot, (size_t)N * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&h->pair_env, (size_t)N * sizeof(int)));
  { const char* e = getenv("RP_HV_WAVES"); h->hv_waves = e ? atoi(e) : 0; }
  CREATE_CHK(hipMalloc((void**)&h->hv_list, (size_t)N * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&h->hv_cnt, 2 * RP_MAX_GROUPS * sizeof(int)));
  CREATE_CHK(hipMemset(h->hv_cnt, 0, 2 * RP_MAX_GROUPS * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&h->member[0], (size_t)N * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&h->member[1], (size_t)N * sizeof(int)));
  {
    const float (*hv)[4]; const int *hoff, *hcnt;
    const int nhv = rp_hull_tables(d->kind, &hv, &hoff, &hcnt);
    if (nhv > 0) {
      CREATE_CHK(hipMalloc((void**)&h->hullv, (size_t)nhv * 4 * sizeof(float)));
      CREATE_CHK(hipMemcpy(h->hullv, hv, (size_t)nhv * 4 * sizeof(float), hipMemcpyHostToDevice));
      const bool off = getenv("RP_NO_HULL") != nullptr;      /* timing / model studies only: arm links as their OBBs everywhere (round 2's contacts) */
      for (int c = 0; c < RP_MAX_COL; c++) { d->hull_off[c] = hoff[c]; d->hull_cnt[c] = off ? 0 : hcnt[c]; }
      /* the candidate tables: the baked lists hold vertex numbers; the kernels read (x, y, z, number) in one 16-byte load */
      const unsigned short* cidx; const int *coff, *cfirst; int ctotal = 0;
      const int ncoff = rp_hcell_tables(d->kind, &cidx, &coff, &cfirst, &ctotal);
      for (int c = 0; c < RP_MAX_COL; c++) d->hcell_first[c] = -1;
      if (ncoff <= 0) {      /*  hulls without candidate tables - a new kind, a bake that went wrong: the narrowphase would read through a null table */
        for (int c = 0; c < RP_MAX_COL; c++)
          if (d->hull_cnt[c] > 0) { snprintf(g_err, 256, "rp_create: collider %d collides as a hull of %d vertices but the model has no support-vertex candidate tables (rp_hullcells_gen.h)", c, d->hull_cnt[c]); e = hipErrorInvalidValue; goto fail; }
      }
      if (ncoff > 0) {
        std::vector<float> cv((size_t)ctotal * 4, 0.f);
        std::vector<char> done((size_t)ncoff, 0);
        for (int c = 0; c < RP_MAX_COL; c++) {
          d->hcell_first[c] = hcnt[c] > 0 ? cfirst[c] : -1;
          if (d->hull_cnt[c] > 0 && cfirst[c] < 0) { snprintf(g_err, 256, "rp_create: collider %d collides as a hull but has no candidate table", c); e = hipErrorInvalidValue; goto fail; }
          if (hcnt[c] <= 0 || cfirst[c] < 0) continue;
          const bool first_user = !done[cfirst[c]];
          done[cfirst[c]] = 1;
          for (int k = coff[cfirst[c]]; k < coff[cfirst[c] + RP_HCELL_N]; k++) {
            const int vi = cidx[k];
            if (vi >= hcnt[c]) {      /* (checked for EVERY collider that shares the table, not only the first) */ snprintf(g_err, 256, "rp_create: the candidate table refers to vertex %d of a %d-vertex hull", vi, hcnt[c]); e = hipErrorInvalidValue; goto fail; }
            if (!first_user) continue;
            const float* v = hv[hoff[c] + vi];
            cv[4 * (size_t)k] = v[0]; cv[4 * (size_t)k + 1] = v[1]; cv[4 * (size_t)k + 2] = v[2]; memcpy(&cv[4 * (size_t)k + 3], &vi, 4);
          }
        }
        CREATE_CHK(hipMalloc((void**)&h->hcv, cv.size() * sizeof(float)));
        CREATE_CHK(hipMemcpy(h->hcv, cv.data(), cv.size() * sizeof(float), hipMemcpyHostToDevice));
        CREATE_CHK(hipMalloc((void**)&h->hco, (size_t)ncoff * sizeof(int)));
        CREATE_CHK(hipMemcpy(h->hco, coff, (size_t)ncoff * sizeof(int), hipMemcpyHostToDevice));
      }
    }
    {      /* the hulls' face planes for the ray caster: baked in the body frame, used in the collider's (x_body = Rc x_col + pc: n_col = Rc^T n, w_col = w + n . pc) */
      const float (*pl)[4]; const int *poff, *pcnt;
      const int npl = rp_hplane_tables(d->kind, &pl, &poff, &pcnt);
      if (npl > 0 && nhv > 0 && getenv("RP_NO_HULL") == nullptr) {
        std::vector<float> hp((size_t)npl * 4, 0.f);
        std::vector<char> done((size_t)npl, 0);
        for (int c = 0; c < RP_MAX_COL; c++) {
          d->hpl_off[c] = poff[c]; d->hpl_cnt[c] = hcnt[c] > 0 ? pcnt[c] : 0;
          if (d->hpl_cnt[c] <= 0) continue;
          if (done[poff[c]]) { d->hpl_cnt[c] = 0; continue; }      /* (a plane list serves ONE collider frame; no model shares one between two) */
          done[poff[c]] = 1;
          const float* Rc = d->col_rot[c]; const float* pc = d->col_pos[c];
          for (int k = poff[c]; k < poff[c] + pcnt[c]; k++) {
            const float* n = pl[k];
            hp[4 * (size_t)k] = Rc[0] * n[0] + Rc[3] * n[1] + Rc[6] * n[2];
            hp[4 * (size_t)k + 1] = Rc[1] * n[0] + Rc[4] * n[1] + Rc[7] * n[2];
            hp[4 * (size_t)k + 2] = Rc[2] * n[0] + Rc[5] * n[1] + Rc[8] * n[2];
            hp[4 * (size_t)k + 3] = n[3] + n[0] * pc[0] + n[1] * pc[1] + n[2] * pc[2];
          }
        }
        CREATE_CHK(hipMalloc((void**)&h->hpl, hp.size() * sizeof(float)));
        CREATE_CHK(hipMemcpy(h->hpl, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice));
      }
    }
    d->hullv = h->hullv; d->hcv = h->hcv; d->hco = h->hco; d->hpl = h->hpl;
    if (!(cfg->flags & RP_CFG_STATELESS_CONTACTS) && !(cfg->flags & RP_CFG_CONTACT_MARGIN) && getenv("RP_STATELESS") == nullptr) {      /* (a uniform contact margin is a stateless-model study: it keeps the stateless contacts) */
      CREATE_CHK(hipMalloc((void**)&h->pmcache, (size_t)N * PMC_FLOATS * sizeof(float)));
      CREATE_CHK(hipMemset(h->pmcache, 0, (size_t)N * PMC_FLOATS * sizeof(float)));
      d->persist = 1; d->pmcache = h->pmcache;
    }
    d->gjk = ((cfg->flags & RP_CFG_OBB_EDGES) || getenv("RP_NO_GJK") != nullptr) ? 0 : 1;      /* (oracle RPO_RULE_GJK: the default; RP_NO_GJK=1: the tools' switch to round 3's OBB edges) */
    {      /* oracle RPO_RULE_EPA: the Panda kinds' default (rpo_create); RP_CFG_HULL_EPA / RP_CFG_NO_HULL_EPA or the tools' RP_EPA=1 / RP_NO_EPA=1 force it */
      int epa = (SPEC[cfg->env_kind].model == 'U' || SPEC[cfg->env_kind].model == 'R') ? 0 : 1;
      if ((cfg->flags & RP_CFG_HULL_EPA) || getenv("RP_EPA") != nullptr) epa = 1;
      if ((cfg->flags & RP_CFG_NO_HULL_EPA) || getenv("RP_NO_EPA") != nullptr) epa = 0;
      d->epa = d->gjk ? epa : 0;
    }
    d->spec_limits = (cfg->flags & RP_CFG_SPECULATIVE_LIMITS) ? 1 : 0;
    if (getenv("RP_NO_SPIN") != nullptr)                     /* timing / model studies only: no torsional friction rows */
      for (int c = 0; c < RP_MAX_COL; c++) d->col_spin[c] = 0.f;
  }
  {      /* the per-env dynamics table, every row the bake's: each object's friction (uniform over its colliders in the bake: the first one's), each free body's mass */
    if (d->n_obj > RP_MAX_OBJ) { snprintf(g_err, 256, "rp_create: %d collision objects, at most %d", d->n_obj, RP_MAX_OBJ); rc = RP_ERR_UNSUPPORTED; goto fail; }
    const int nd = d->n_obj + d->n_free;
    float row[RP_MAX_OBJ + RP_MAX_FREE];
    for (int c = d->n_col - 1; c >= 0; c--) row[d->col_obj[c]] = d->col_friction[c];
    for (int f = 0; f < d->n_free; f++) row[d->n_obj + f] = d->free_mass[f];
    CREATE_CHK(hipMalloc((void**)&h->dyn, (size_t)(N + 1) * nd * sizeof(float)));      /* (+ one row behind the table: the bake's, broadcast from there) */
    const float* base = h->dyn + (size_t)N * nd;
    CREATE_CHK(hipMemcpy((void*)base, row, nd * sizeof(float), hipMemcpyHostToDevice));
    launch_table_set(h, h->dyn, {base, base + d->n_obj, nullptr, d->n_obj, d->n_free, 0}, 0, 1, nullptr, nullptr);
    CREATE_CHK(hipGetLastError());
    d->dyn = h->dyn;
  }
  {      /* the per-env wrench table: nothing pushes until rp_set_wrench says so */
    const size_t bytes = (size_t)N * (d->nbody - 1) * 6 * sizeof(float);
    CREATE_CHK(hipMalloc((void**)&h->wrench, bytes));
    CREATE_CHK(hipMemset(h->wrench, 0, bytes));
    d->wrench = h->wrench;
  }
  {      /* the per-env actuation table, every row the constants the kernels had: gravity (0, 0, -9.8), motor gain 1, motor strength 1 */
    const int na = d->n_arm, W = 3 + 2 * na;
    float row[3 + 2 * RP_MAX_ARM];
    row[0] = 0.f; row[1] = 0.f; row[2] = K_GRAVITY;
    for (int i = 0; i < 2 * na; i++) row[3 + i] = 1.f;
    CREATE_CHK(hipMalloc((void**)&h->act, (size_t)(N + 1) * W * sizeof(float)));      /* (+ one row behind the table: the default row, broadcast from there) */
    const float* base = h->act + (size_t)N * W;
    CREATE_CHK(hipMemcpy((void*)base, row, W * sizeof(float), hipMemcpyHostToDevice));
    launch_table_set(h, h->act, {base, base + 3, base + 3 + na, 3, na, na}, 0, 1, nullptr, nullptr);
    CREATE_CHK(hipGetLastError());
    d->act = h->act;
  }
  CREATE_CHK(hipMemcpy(h->dev_model, &h->host_model, sizeof(DevModel), hipMemcpyHostToDevice));
  CREATE_CHK(hipEventCreate(&h->ev0));
  CREATE_CHK(hipEventCreate(&h->ev1));
  {
    const char* g = getenv("RP_STEP_GROUPS");
    h->groups = g ? atoi(g) : 3;      /* 3 group streams + nothing else stays within the 4 hardware queues ROCm multiplexes onto */
    if (h->groups < 1) h->groups = 1;
    if (h->groups > RP_MAX_GROUPS) h->groups = RP_MAX_GROUPS;
    { const char* cb = getenv("RP_CHAIN_BLOCKS"); h->chain_blocks = cb ? (atoi(cb) > 0 ? atoi(cb) : 1) : 1024; }      /* k_chain's grid: 256 CUs x 4 blocks of 40 KB LDS and 2 x 217 VGPRs - everything resident at once */
    CREATE_CHK(hipEventCreateWithFlags(&h->gfork, hipEventDisableTiming));
    /* RP_GROUP_SPLIT="30,30,40": relative group sizes, heaviest group first (default: 25,35,40 for 3 groups, equal otherwise).  Stream priorities for the heavy
     * group were tried and lose (2.69 vs 2.61 ms per step). */
    const char* sp = getenv("RP_GROUP_SPLIT");
    for (int i = 0; i < RP_MAX_GROUPS; i++) h->gsplit[i] = 0;
    if (sp) { int i = 0; while (*sp && i < RP_MAX_GROUPS) { h->gsplit[i++] = atoi(sp); while (*sp && *sp != ',') sp++; if (*sp == ',') sp++; } }
    for (int i = 0; i < RP_MAX_GROUPS; i++) {
      CREATE_CHK(hipStreamCreateWithFlags(&h->gstream[i], hipStreamNonBlocking));
      CREATE_CHK(hipEventCreateWithFlags(&h->gjoin[i], hipEventDisableTiming));
    }
  }
  {      /* rp_step_autoreset: counters start at 0; k_autoreset's grid is what is resident at once (it takes envs off a list, so more blocks would only wait) */
    CREATE_CHK(hipMalloc((void**)&h->ep_steps, (size_t)N * sizeof(int)));
    CREATE_CHK(hipMemset(h->ep_steps, 0, (size_t)N * sizeof(int)));
    CREATE_CHK(hipMalloc((void**)&h->ar_list, (size_t)N * sizeof(int)));
    CREATE_CHK(hipMalloc((void**)&h->ar_ctl, 2 * sizeof(int)));
    const char* eb = getenv("RP_AUTORESET_EPB");
    h->ar_epb = eb ? atoi(eb) : 1;
    if (h->ar_epb < 1) h->ar_epb = 1;
    if (h->ar_epb > 4) h->ar_epb = 4;
    int cus = 0, per_cu = 0;
    CREATE_CHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
    CREATE_CHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_autoreset, 64 * SOLVE_WAVES, 0));
    const char* ab = getenv("RP_AUTORESET_BLOCKS");
    h->ar_grid = ab && atoi(ab) > 0 ? atoi(ab) : max(cus, 1) * max(per_cu, 1);
    h->ar_grid = min(h->ar_grid, (N + h->ar_epb - 1) / h->ar_epb);
    CREATE_CHK(hipMalloc((void**)&h->ar_pair, (size_t)4 * h->ar_grid * sizeof(int)));
    h->ar_max_steps = 0; h->ar_when = RP_AR_FAULT;
    /* the reset table's rows and ranks; no table yet.  k_autoreset_to: one wave per env, as many as are resident at once (it strides over the list) */
    const size_t nwv = (size_t)(N + 255) / 256 * 4;
    CREATE_CHK(hipMalloc((void**)&h->rt_cursor, sizeof(int)));
    CREATE_CHK(hipMemset(h->rt_cursor, 0, sizeof(int)));
    CREATE_CHK(hipMalloc((void**)&h->rt_env_row, (size_t)N * sizeof(int)));
    CREATE_CHK(hipMemset(h->rt_env_row, 0xff, (size_t)N * sizeof(int)));
    CREATE_CHK(hipMalloc((void**)&h->rt_wave_bal, nwv * sizeof(unsigned long long)));
    CREATE_CHK(hipMalloc((void**)&h->rt_wave_row, nwv * sizeof(int)));
    CREATE_CHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_autoreset_to, 64, 0));
    h->rt_grid = min(max(cus, 1) * max(per_cu, 1), N);
  }
  hipLaunchKernelGGL(k_init, dim3((N + 255) / 256), dim3(256), 0, 0, h->dev_model, h->state, N);
  CREATE_CHK(hipGetLastError());
  CREATE_CHK(hipDeviceSynchronize());
#undef CREATE_CHK
  *out = h;
  return RP_OK;
fail:
  (void)hipGetLastError();
  destroy_handle(h);
  return rc;
}

int rp_destroy(rp_handle h) {
  if (!h) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  hipDeviceSynchronize();
  destroy_handle(h);
  return RP_OK;
}

int rp_get_dims(rp_handle h, rp_dims* d) {
  if (!h || !d) return RP_ERR_ARG;
  const DevModel* m = &h->host_model;
  d->obs_quat = m->n_obs; d->achieved_goal = m->n_ag; d->desired_goal = m->n_ag; d->controllable_achieved_goal = 4;
  d->full_positional_state = m->n_fps; d->joints = 8; d->velocity = 6; d->observation = m->n_observation;
  d->target_poses = m->n_target; d->action = m->n_action;
  return RP_OK;
}

/* playEnv.reset() for the masked envs through the split pipeline: rounds of { gather the envs that still have a settle phase
 * ahead, sample their objects, 100 x (k_settle_prep, k_settle_solve: k_prep2 / k_solve2 under other names) over the dense scratch range, finish / re-sample / next attempt }.
 * One host sync per round (the pending count sizes the launches); a round is ~100 substeps, most resets take 1-3 rounds, the
 * unluckiest env of a large batch a few more (play ids repeat the reset while the drawn goal is already satisfied). */
static int reset_split(rp_handle h, const uint8_t* mask, const rp_out* out, hipStream_t s) {
  const int N = h->cfg.num_envs;
  if (!h->rs_state) {
    if (hipMalloc((void**)&h->rs_state, (size_t)N * RP_REC_FLOATS * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&h->rs_idx, (size_t)N * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&h->rs_meta, (size_t)N * sizeof(int4)) != hipSuccess ||
        hipMalloc((void**)&h->rs_count, sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&h->rs_sort_cnt, (size_t)2 * SORT_BINS * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&h->rs_sort_slot, (size_t)N * sizeof(int)) != hipSuccess ||
        hipMalloc((void**)&h->rs_pair, (size_t)N * sizeof(int)) != hipSuccess ||
        hipHostMalloc((void**)&h->rs_count_host, sizeof(int)) != hipSuccess) {
      snprintf(h->err, 256, "rp_reset: scratch allocation failed"); return RP_ERR_HIP;
    }
  }
  const OutPtrs op = to_ptrs(out);
  const uint64_t seed = h->cfg.seed;
  const uint32_t off = (uint32_t)h->cfg.env_offset;
  hipLaunchKernelGGL(k_reset_mark, dim3((N + 255) / 256), dim3(256), 0, s, mask, h->rs_meta, N);
  int* cnt[2] = {h->rs_sort_cnt, h->rs_sort_cnt + SORT_BINS};
  h->reset_rounds = 0;
  bool exhausted = true;            /* the loop ran out of rounds (otherwise it left through M <= 0, which already proved that nothing is pending) */
  for (int round = 0; round < 64 * 9; round++) {
    hipLaunchKernelGGL(k_reset_list, dim3(1), dim3(64), 0, s, h->rs_meta, h->rs_idx, h->rs_count, N);
    HIPCHK(h, hipMemcpyAsync(h->rs_count_host, h->rs_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const int M = *h->rs_count_host;
    if (M <= 0) { exhausted = false; break; }
    h->reset_rounds++;
    hipLaunchKernelGGL(k_reset_sample, dim3(M), dim3(64), 0, s, h->dev_model, h->state, h->rs_state, h->rs_idx, M, seed, off);
    hipLaunchKernelGGL(k_sort_init, dim3((max(M, SORT_BINS) + 255) / 256), dim3(256), 0, s, cnt[0], h->rs_sort_slot, 0, M);
    int par = 0;
    for (int i = 0; i < K_NSETTLE; i++) {
      hipLaunchKernelGGL(k_settle_prep, dim3(M), dim3(PREP_THREADS), 0, s, h->dev_model, h->rs_state, h->ws, 0, M, cnt[par], cnt[par ^ 1], h->rs_sort_slot, h->rs_pair, (const int*)nullptr, (const int*)h->rs_idx, h->debug_flags & 1);
      hipLaunchKernelGGL(k_settle_solve, dim3((M + 2 * SOLVE_WAVES - 1) / (2 * SOLVE_WAVES)), dim3(64 * SOLVE_WAVES), 0, s, h->dev_model, h->rs_state, h->ws, 0, M, h->rs_pair, cnt[par ^ 1], h->rs_sort_slot, h->debug_flags);
      par ^= 1;
    }
    hipLaunchKernelGGL(k_reset_finish, dim3(M), dim3(64), 0, s, h->dev_model, h->rs_state, h->state, h->rs_idx, h->rs_meta, op, M, seed, off);
    HIPCHK(h, hipGetLastError());
  }
  /* the round budget is 9 object re-samples x 64 attempts, which k_reset_finish's own caps (depth < 8, attempt < 64) cannot
   * exceed; if envs are pending all the same, say so instead of handing back half-reset records */
  if (!exhausted) return RP_OK;
  hipLaunchKernelGGL(k_reset_list, dim3(1), dim3(64), 0, s, h->rs_meta, h->rs_idx, h->rs_count, N);
  HIPCHK(h, hipMemcpyAsync(h->rs_count_host, h->rs_count, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (*h->rs_count_host > 0) {
    hipLaunchKernelGGL(k_reset_flag_pending, dim3((N + 255) / 256), dim3(256), 0, s, h->rs_meta, op.status, N);
    snprintf(h->err, 256, "rp_reset: %d envs still pending after %d rounds (status bit 4 set)", *h->rs_count_host, h->reset_rounds);
    return RP_ERR_INCOMPLETE;
  }
  return RP_OK;
}

static int reset_impl(rp_handle h, const float* o, int32_t n_o, const uint8_t* mask, const rp_out* out, void* stream) {
  DevGuard guard(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  int N = h->cfg.num_envs;
  if (h->timers_on) hipEventRecord(h->ev0, s);
  hipLaunchKernelGGL(k_episode_zero, dim3((N + 255) / 256), dim3(256), 0, s, mask, h->ep_steps, N);      /* the reset envs start a new episode */
  if (!o && h->fused != 1) {
    int rc = reset_split(h, mask, out, s);
    if (rc == RP_ERR_INCOMPLETE) image_pass(h, false, nullptr, mask, s);      /* (the rows are written, pending envs included: the images show the state they have) */
    if (rc != RP_OK) return rc;
  } else {          /* reset(o) has no settle phase; the fused path keeps everything in one kernel */
    hipLaunchKernelGGL(k_reset, dim3(N), dim3(64), 0, s, h->dev_model, h->state, mask, to_ptrs(out), N, h->cfg.seed, (uint32_t)h->cfg.env_offset, o, (int)n_o);
  }
  image_pass(h, false, nullptr, mask, s);      /* rp_set_image_obs: the images of the envs whose rows were written */
  HIPCHK(h, hipGetLastError());
  if (h->timers_on) { hipEventRecord(h->ev1, s); hipEventSynchronize(h->ev1); hipEventElapsedTime(&h->timers.last_reset_ms, h->ev0, h->ev1); }
  return RP_OK;
}

int rp_reset(rp_handle h, const uint8_t* mask, const rp_out* out, void* stream) {
  if (!h) return RP_ERR_ARG;
  return reset_impl(h, nullptr, 0, mask, out, stream);
}

/* entries of o that reset(o) reads: reset_object_pos(obs) reads object b at o[11 + 10 b : 18 + 10 b] (use_orientation) or o[7 + 6 b : 10 + 6 b] (environments.py:544-556) */
static int reset_to_need(const DevModel* m) {
  return m->num_objects > 0 ? (m->use_orientation ? 18 + 10 * (m->num_objects - 1) : 10 + 6 * (m->num_objects - 1))
                            : (m->use_orientation ? (m->return_velocity ? 10 : 7) : 3);
}

int rp_reset_to(rp_handle h, const float* o, int32_t n_o, const uint8_t* mask, const rp_out* out, void* stream) {
  if (!h || !o) return RP_ERR_ARG;
  const int need = reset_to_need(&h->host_model);
  if (n_o < need) { snprintf(h->err, 256, "rp_reset_to: o has %d entries per env, this env reads %d", n_o, need); return RP_ERR_ARG; }
  return reset_impl(h, o, n_o, mask, out, stream);
}

int rp_reset_goal(rp_handle h, const float* goal, const uint8_t* mask, void* stream) {
  if (!h) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  int N = h->cfg.num_envs;
  hipLaunchKernelGGL(k_reset_goal, dim3(N), dim3(64), 0, (hipStream_t)stream, h->dev_model, h->state, goal, mask, N, h->cfg.seed,
                     (uint32_t)h->cfg.env_offset);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

/* the split pipeline's G env groups: places [b[g], b[g + 1]) of the load ranking */
static GroupBounds split_groups(rp_handle h, int G, int N) {
  GroupBounds gb;
  long long tot = 0, acc = 0;
  static const int split3[3] = {25, 35, 40};     /* default for 3 groups: the heavy group smaller (2.54 vs 2.59 ms per step, equal thirds) */
  const int* split = h->gsplit;
  if (h->gsplit[0] <= 0 && G == 3) split = split3;
  for (int g = 0; g < G; g++) tot += split[g] > 0 ? split[g] : 0;
  bool custom = tot > 0;
  for (int g = 0; g < G && custom; g++) if (split[g] <= 0) custom = false;
  gb.b[0] = 0;
  for (int g = 0; g < G; g++) {
    acc += custom ? split[g] : 1;
    gb.b[g + 1] = (int)((long long)N * acc / (custom ? tot : G));
  }
  for (int g = G + 1; g <= RP_MAX_GROUPS; g++) gb.b[g] = N;
  return gb;
}

/* rp_step without the image observations: rp_step_autoreset draws its own, around the resets */
static int step_impl(rp_handle h, const float* action, const rp_out* out, void* stream) {
  if (!h || !action) { if (h) snprintf(h->err, 256, "rp_step: action is NULL"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  int N = h->cfg.num_envs;
  if (h->timers_on && h->fused == 1) hipEventRecord(h->ev0, s);
  if (h->fused == 1) {
    hipLaunchKernelGGL(k_step, dim3(N), dim3(64), 0, s, h->dev_model, h->state, action, to_ptrs(out), N);
  } else if (h->fused == 2) {
    /* round 4's experiment (rp_set_fused(h, 2)): the twelve substeps in ONE launch, k_chain - blocks of two waves own four envs each (in the load ranking's order) for
     * the whole step.  Ranking, action kernel, the chain, observations: four launches on the caller's stream */
    OutPtrs op = to_ptrs(out);
    GroupBounds gb;
    gb.b[0] = 0;
    for (int g = 1; g <= RP_MAX_GROUPS; g++) gb.b[g] = N;
    if (h->sort_G == 0) hipLaunchKernelGGL(k_member_identity, dim3((N + 255) / 256), dim3(256), 0, s, h->member[h->member_cur], N, h->hv_cnt);
    else {
      hipLaunchKernelGGL(k_member, dim3(1), dim3(1024), 0, s, h->member[h->member_cur], h->member[h->member_cur ^ 1], h->sort_cnt + (size_t)h->sort_par * RP_MAX_GROUPS * SORT_BINS,
                         h->sort_slot, N, h->sort_G, h->gb, 1, gb, h->hv_cnt);
      h->member_cur ^= 1;
    }
    const int* member = h->member[h->member_cur];
    int* cnt_next = h->sort_cnt + (size_t)(h->sort_par ^ 1) * RP_MAX_GROUPS * SORT_BINS;      /* the last substep's load classes: the next step's ranking */
    HIPCHK(h, hipMemsetAsync(cnt_next, 0, SORT_BINS * sizeof(int), s));
    hipLaunchKernelGGL(k_action, dim3((N + 3) / 4), dim3(64), 0, s, h->dev_model, h->state, action, op.target_poses, 0, N, member);
    const int nq = (N + 3) / 4;
    const int blocks = min(nq, h->chain_blocks);          /* 256 CUs x 4 blocks of 40 KB LDS and 2 x 217 VGPRs: everything resident at once */
    hipLaunchKernelGGL(k_chain, dim3(blocks), dim3(64 * SOLVE_WAVES), 0, s, h->dev_model, h->state, h->ws, N, member, h->pair_env, cnt_next, h->sort_slot, K_NSUB, h->debug_flags);
    hipLaunchKernelGGL(k_calc_state, dim3(N), dim3(64), 0, s, h->dev_model, h->state, op, 0, N, member);
    h->sort_par ^= 1; h->sort_G = 1; h->gb = gb;
  } else {
    OutPtrs op = to_ptrs(out);
    hipEvent_t* ev = h->pool ? h->pool + (size_t)h->pool_next * EV_PER_STEP : nullptr;
    /* Env groups: substeps of different envs are independent, so the envs are cut into `groups` contiguous ranges and
     * each range runs its own 25-kernel chain on its own stream; the tail of one group's k_solve2 (its heaviest wave)
     * overlaps with the other groups' kernels.  Per-launch timing (rp_enable_timers) uses one group so that the event
     * pairs bracket exactly one kernel each. */
    int G = ev ? 1 : h->groups;
    if (G > (N + 63) / 64) G = (N + 63) / 64;
    int e = 2;
#ifdef RP_SYNC_DEBUG      /* debugging builds: synchronise after every launch of the chain and say which one died */
#define TIMED(launch) do { fprintf(stderr, "[rp sync] launching %.40s\n", #launch); fflush(stderr); launch; hipError_t e_ = hipDeviceSynchronize(); fprintf(stderr, "[rp sync]   -> %d\n", (int)e_); fflush(stderr); } while (0)
#else
#define TIMED(launch) do { if (ev) hipEventRecord(ev[e++], gs); launch; if (ev) hipEventRecord(ev[e++], gs); } while (0)
#endif
    /* groups by load: rank all envs by the load class of the latest k_solve2 and cut the ranking into the G groups */
    const GroupBounds gb = split_groups(h, G, N);
    const int* member = h->member[h->member_cur];
    if (h->sort_G == 0) {
      hipLaunchKernelGGL(k_member_identity, dim3((N + 255) / 256), dim3(256), 0, s, h->member[h->member_cur], N, h->hv_cnt);
    } else {
      hipLaunchKernelGGL(k_member, dim3(1), dim3(1024), 0, s, member, h->member[h->member_cur ^ 1], h->sort_cnt + (size_t)h->sort_par * RP_MAX_GROUPS * SORT_BINS,
                         h->sort_slot, N, h->sort_G, h->gb, G, gb, h->hv_cnt);
      h->member_cur ^= 1;
      member = h->member[h->member_cur];
    }
    if (G > 1) hipEventRecord(h->gfork, s);
    /* The groups' chains are enqueued ROUND-ROBIN, one launch per group at a time: a chain is 26 dependent launches and its length (not the
     * machine's width) sets the step time at N = 4096, so all chains have to start at once - enqueued group by group, the last group's chain
     * started a whole group's worth of host launch time late (2.38 -> 2.1x ms per step).  Same kernels, same arguments, same order inside
     * every stream. */
    struct GroupCtx { hipStream_t gs; int e0, e1, ng, nab, hb; int* gcnt[2]; int* hvc[2]; } gc[RP_MAX_GROUPS];
    const int par0 = h->sort_par;
    for (int g = 0; g < G; g++) {
      GroupCtx& c = gc[g];
      /* group 0 stays on the caller's stream; a fourth group takes gstream[0], the stream created first: with the default four hardware queues of a process it is
       * the one that has a queue to itself (the kernel trace shows queues 1, 3, 4 for three groups and 2 for gstream[0]); gstream[3] shares one, and two chains on
       * one queue run one after the other (3.6 ms per step).  Four groups are 0.7 % faster than three and leave no queue for anybody else: the default stays 3 */
      c.gs = g == 0 ? s : h->gstream[g == 3 ? 0 : g];
      c.e0 = gb.b[g]; c.e1 = gb.b[g + 1]; c.ng = c.e1 - c.e0; c.nab = (c.ng + 3) / 4;      /* action blocks of 64 threads: one env per 16 lanes (k_action_prep: 128 threads, half as many) */
      /* env pairing of this group: k_solve2 ranks its envs by load class (histogram, double-buffered), the next k_prep2
       * turns the ranks into the table the next k_solve2 reads */
      c.gcnt[0] = h->sort_cnt + (size_t)g * SORT_BINS; c.gcnt[1] = h->sort_cnt + (size_t)(RP_MAX_GROUPS + g) * SORT_BINS;
      /* the heavy envs of a substep (1 - 2 % of the envs: a grasp, a push, a crowded drawer) are listed by its k_prep2 and solved one per wave by worker blocks at the head
       * of k_solve2's grid: an eighth of the group's envs' worth of waves (a longer list is walked in strides) */
      c.hvc[0] = h->hv_cnt + g; c.hvc[1] = h->hv_cnt + RP_MAX_GROUPS + g;
      c.hb = (h->debug_flags & 1) ? c.ng : (h->hv_waves > 0 ? h->hv_waves : max((c.ng + 1) / 2, 16));      /* worker blocks: one heavy env each at a time (debug flag 1: every env is on the list) */
      if (c.gs != s) hipStreamWaitEvent(c.gs, h->gfork, 0);
      if (ev) hipEventRecord(ev[0], c.gs);
      if (h->sort_G == 0) hipLaunchKernelGGL(k_sort_init, dim3((max(c.ng, SORT_BINS) + 255) / 256), dim3(256), 0, c.gs, c.gcnt[par0], h->sort_slot, c.e0, c.ng);
    }
    /* first substep: action kernel and first k_prep2 in one launch (k_action_prep), the motor rows rebuilt by the k_solve2 after
     * it (flag bit 1); with per-launch timers on (one group), the kernels stay apart so that every event pair brackets one of them */
    if (ev) { hipStream_t gs = gc[0].gs; TIMED(hipLaunchKernelGGL(k_action, dim3(gc[0].nab), dim3(64), 0, gs, h->dev_model, h->state, action, op.target_poses, gc[0].e0, gc[0].e1, member)); }
    int par = par0;
    for (int sub = 0; sub < K_NSUB; sub++) {
      const bool merged = !ev && sub == 0;
      for (int g = 0; g < G; g++) {
        const GroupCtx& c = gc[g];
        hipStream_t gs = c.gs;
        if (merged) {
#ifdef RP_SYNC_DEBUG
          fprintf(stderr, "[rp sync] before k_action_prep: %d\n", (int)hipDeviceSynchronize()); fflush(stderr);
#endif
          hipLaunchKernelGGL(k_action_prep, dim3((c.ng + 7) / 8 + c.ng), dim3(PREP_THREADS), 0, gs, h->dev_model, h->state, h->ws, c.e0, c.e1, c.gcnt[par], c.gcnt[par ^ 1], h->sort_slot,
                             h->pair_env, member, action, op.target_poses, (c.ng + 7) / 8, c.hvc[sub & 1], c.hvc[(sub & 1) ^ 1], h->hv_list, h->debug_flags & 1);
#ifdef RP_SYNC_DEBUG
          fprintf(stderr, "[rp sync] after k_action_prep: %d\n", (int)hipDeviceSynchronize()); fflush(stderr);
#endif
        } else
          TIMED(hipLaunchKernelGGL(k_prep2, dim3(c.ng), dim3(PREP_THREADS), 0, gs, h->dev_model, h->state, h->ws, c.e0, c.e1, c.gcnt[par], c.gcnt[par ^ 1], h->sort_slot, h->pair_env, member,
                                   c.hvc[sub & 1], c.hvc[(sub & 1) ^ 1], h->hv_list, h->debug_flags & 1));
      }
      for (int g = 0; g < G; g++) {
        const GroupCtx& c = gc[g];
        hipStream_t gs = c.gs;
        TIMED(hipLaunchKernelGGL(k_solve2, dim3(c.hb + (c.ng + 2 * SOLVE_WAVES - 1) / (2 * SOLVE_WAVES)), dim3(64 * SOLVE_WAVES), 0, gs, h->dev_model, h->state, h->ws, c.e0, c.e1, h->pair_env, c.gcnt[par ^ 1], h->sort_slot,
                                 h->debug_flags | (merged ? RP_DBG_MOTOR : 0) | RP_DBG_WORKERS, (const int*)c.hvc[sub & 1], (const int*)h->hv_list, c.hb));
      }
      par ^= 1;
    }
    h->sort_par = par; h->sort_G = G; h->gb = gb;
    for (int g = 0; g < G; g++) {
      const GroupCtx& c = gc[g];
      hipStream_t gs = c.gs;
      TIMED(hipLaunchKernelGGL(k_calc_state, dim3(c.ng), dim3(64), 0, gs, h->dev_model, h->state, op, c.e0, c.e1, member));
      if (ev) hipEventRecord(ev[1], gs);
      if (gs != s) hipEventRecord(h->gjoin[g], gs);
    }
    for (int g = 1; g < G; g++) hipStreamWaitEvent(s, h->gjoin[g], 0);
    if (ev) {
      h->pool_next = (h->pool_next + 1) % h->pool_steps;
      if (h->pool_count < h->pool_steps) h->pool_count++;
    }
#undef TIMED
  }
  HIPCHK(h, hipGetLastError());
  if (h->timers_on && h->fused == 1) { hipEventRecord(h->ev1, s); hipEventSynchronize(h->ev1); hipEventElapsedTime(&h->timers.last_step_ms, h->ev0, h->ev1); }
  h->timers.steps++;
  return RP_OK;
}

int rp_step(rp_handle h, const float* action, const rp_out* out, void* stream) {
  int rc = step_impl(h, action, out, stream);
  if (rc != RP_OK || !h->img.n) return rc;
  DevGuard guard(h->cfg.device);
  image_pass(h, false, nullptr, nullptr, (hipStream_t)stream);      /* on the caller's stream, which the group streams have joined */
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_set_autoreset(rp_handle h, int32_t max_episode_steps, uint32_t when) {
  if (!h) return RP_ERR_ARG;
  if (when & ~(uint32_t)(RP_AR_TIME_LIMIT | RP_AR_FAULT | RP_AR_SUCCESS)) { snprintf(h->err, 256, "rp_set_autoreset: unknown bits in when (0x%x)", when); return RP_ERR_ARG; }
  h->ar_max_steps = max_episode_steps; h->ar_when = when;
  return RP_OK;
}

int rp_get_episode_steps(rp_handle h, int32_t* dst, void* stream) {
  if (!h || !dst) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  HIPCHK(h, hipMemcpyAsync(dst, h->ep_steps, (size_t)h->cfg.num_envs * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RP_OK;
}

int rp_set_episode_steps(rp_handle h, const int32_t* src, void* stream) {
  if (!h || !src) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  HIPCHK(h, hipMemcpyAsync(h->ep_steps, src, (size_t)h->cfg.num_envs * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RP_OK;
}

/* rp_step, then on the same stream: k_autoreset_mark (done bits, final_out rows, counters, the list of ending envs) and ONE k_autoreset launch that resets the listed envs
 * (an empty list: its blocks leave at once).  Nothing is read back; the call returns when everything is enqueued.  With rp_set_image_obs: the step does not draw; the
 * terminal pass (the envs with done != 0, by the kernels' selection: their blocks alone do work) stands between the mark and the reset, the observation pass at the end. */
int rp_step_autoreset(rp_handle h, const float* action, const uint8_t* end_mask, const rp_out* out, const rp_out* final_out, int32_t* done, void* stream) {
  if (!h || !action || !done) { if (h) snprintf(h->err, 256, "rp_step_autoreset: action or done is NULL"); return RP_ERR_ARG; }
  if ((h->ar_when & RP_AR_FAULT) && (!out || !out->status)) { snprintf(h->err, 256, "rp_step_autoreset: RP_AR_FAULT reads out.status, which is NULL"); return RP_ERR_ARG; }
  if ((h->ar_when & RP_AR_SUCCESS) && (!out || !out->is_success)) { snprintf(h->err, 256, "rp_step_autoreset: RP_AR_SUCCESS reads out.is_success, which is NULL"); return RP_ERR_ARG; }
  int rc = step_impl(h, action, out, stream);
  if (rc != RP_OK) return rc;
  DevGuard guard(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  const int N = h->cfg.num_envs;
  const OutPtrs op = to_ptrs(out), fp = to_ptrs(final_out);
  HIPCHK(h, hipMemsetAsync(h->ar_ctl, 0, 2 * sizeof(int), s));
  const bool table = h->rt_rows > 0;
  hipLaunchKernelGGL(k_autoreset_mark, dim3((N + 255) / 256), dim3(256), 0, s, h->dev_model, N, (int)h->ar_max_steps, (unsigned)h->ar_when, end_mask, op, fp, done, h->ep_steps,
                     h->ar_list, h->ar_ctl, h->rt_env_row, table ? h->rt_wave_bal : (unsigned long long*)nullptr);
  image_pass(h, true, done, nullptr, s);       /* rp_set_image_obs' terminal pass: the ended envs' last frame, from the state the step left, into final_* */
  if (table) {
    hipLaunchKernelGGL(k_autoreset_rows, dim3(1), dim3(1024), 0, s, (const unsigned long long*)h->rt_wave_bal, (N + 63) / 64, h->rt_wave_row, h->rt_cursor, h->rt_rows);
    hipLaunchKernelGGL(k_autoreset_to, dim3(h->rt_grid), dim3(64), 0, s, h->dev_model, h->state, (const int*)h->ar_list, (const int*)h->ar_ctl,
                       (const unsigned long long*)h->rt_wave_bal, (const int*)h->rt_wave_row, (const float*)h->rt_tab, h->rt_rows, h->rt_n_o, h->rt_env_row, op, h->cfg.seed,
                       (uint32_t)h->cfg.env_offset);
  } else {
    hipLaunchKernelGGL(k_autoreset, dim3(h->ar_grid), dim3(64 * SOLVE_WAVES), 0, s, h->dev_model, h->state, h->ws, (const int*)h->ar_list, h->ar_ctl, h->ar_pair, op, h->cfg.seed,
                       (uint32_t)h->cfg.env_offset, h->ar_epb, h->debug_flags);
  }
  image_pass(h, false, nullptr, nullptr, s);   /* ... and its observation pass: every env, the ended ones at their new episode's first frame */
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

/* The table is copied into library memory on `stream`.  The device is synchronised first: steps still in flight (on any stream) may read the table this call replaces. */
int rp_set_reset_table(rp_handle h, const float* o, int32_t rows, int32_t n_o, void* stream) {
  if (!h) return RP_ERR_ARG;
  if (rows < 0) { snprintf(h->err, 256, "rp_set_reset_table: rows = %d is negative", rows); return RP_ERR_ARG; }
  if (rows > 0) {
    if (!o) { snprintf(h->err, 256, "rp_set_reset_table: o is NULL with rows = %d", rows); return RP_ERR_ARG; }
    const int need = reset_to_need(&h->host_model);
    if (n_o < need) { snprintf(h->err, 256, "rp_set_reset_table: o has %d entries per row, this env reads %d", n_o, need); return RP_ERR_ARG; }
  }
  DevGuard guard(h->cfg.device);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipFree(h->rt_tab));
  h->rt_tab = nullptr; h->rt_rows = 0; h->rt_n_o = 0;
  HIPCHK(h, hipMemsetAsync(h->rt_cursor, 0, sizeof(int), s));
  if (rows == 0) return RP_OK;
  const size_t bytes = (size_t)rows * (size_t)n_o * sizeof(float);
  HIPCHK(h, hipMalloc((void**)&h->rt_tab, bytes));
  HIPCHK(h, hipMemcpyAsync(h->rt_tab, o, bytes, hipMemcpyDeviceToDevice, s));
  h->rt_rows = rows; h->rt_n_o = n_o;
  return RP_OK;
}

int rp_get_dynamics_dims(rp_handle h, int32_t* n_obj, int32_t* n_free) {
  if (!h || !n_obj || !n_free) return RP_ERR_ARG;
  *n_obj = h->host_model.n_obj; *n_free = h->host_model.n_free;
  return RP_OK;
}

/* enqueued on `stream` like a step: a step queued after it on the same stream sees the new values, one queued before it the old ones */
int rp_set_dynamics(rp_handle h, const float* friction, const float* mass, int32_t rows, const uint8_t* mask, void* stream) {
  if (!h) return RP_ERR_ARG;
  if (!friction && !mass) { snprintf(h->err, 256, "rp_set_dynamics: friction and mass are both NULL"); return RP_ERR_ARG; }
  return table_set(h, "rp_set_dynamics", h->dyn, {friction, mass, nullptr, h->host_model.n_obj, h->host_model.n_free, 0}, 0, rows, mask, stream);
}

int rp_get_dynamics(rp_handle h, float* friction, float* mass, void* stream) {
  if (!h || (!friction && !mass)) { if (h) snprintf(h->err, 256, "rp_get_dynamics: friction and mass are both NULL"); return RP_ERR_ARG; }
  return table_get(h, h->dyn, {friction, mass, nullptr, h->host_model.n_obj, h->host_model.n_free, 0}, stream);
}

int rp_get_wrench_dims(rp_handle h, int32_t* n_arm, int32_t* n_free, int32_t* n_j1) {
  if (!h || !n_arm || !n_free || !n_j1) return RP_ERR_ARG;
  *n_arm = h->host_model.n_arm; *n_free = h->host_model.n_free; *n_j1 = h->host_model.n_j1;
  return RP_OK;
}

/* enqueued on `stream` like rp_set_dynamics: a step queued after it on the same stream feels the new wrenches from its first substep, one queued before it the old ones */
int rp_set_wrench(rp_handle h, const float* wrench, int32_t rows, const uint8_t* mask, void* stream) {
  if (!h) return RP_ERR_ARG;
  return table_set(h, "rp_set_wrench", h->wrench, {wrench, nullptr, nullptr, 6 * (h->host_model.nbody - 1), 0, 0}, 1, rows, mask, stream);      /* (NULL = zeros) */
}

int rp_get_wrench(rp_handle h, float* wrench, void* stream) {
  if (!h || !wrench) { if (h) snprintf(h->err, 256, "rp_get_wrench: wrench is NULL"); return RP_ERR_ARG; }
  return table_get(h, h->wrench, {wrench, nullptr, nullptr, 6 * (h->host_model.nbody - 1), 0, 0}, stream);
}

int rp_get_actuation_dims(rp_handle h, int32_t* n_arm) {
  if (!h || !n_arm) return RP_ERR_ARG;
  *n_arm = h->host_model.n_arm;
  return RP_OK;
}

/* enqueued on `stream` like rp_set_dynamics: a step queued after it on the same stream runs under the new values from its first substep, one queued before it under the old ones */
int rp_set_actuation(rp_handle h, const float* gravity, const float* motor_gain, const float* motor_strength, int32_t rows, const uint8_t* mask, void* stream) {
  if (!h) return RP_ERR_ARG;
  const int na = h->host_model.n_arm;
  if (!gravity && !motor_gain && !motor_strength) { snprintf(h->err, 256, "rp_set_actuation: gravity, motor_gain and motor_strength are all NULL"); return RP_ERR_ARG; }
  return table_set(h, "rp_set_actuation", h->act, {gravity, motor_gain, motor_strength, 3, na, na}, 0, rows, mask, stream);
}

int rp_get_actuation(rp_handle h, float* gravity, float* motor_gain, float* motor_strength, void* stream) {
  if (!h || (!gravity && !motor_gain && !motor_strength)) { if (h) snprintf(h->err, 256, "rp_get_actuation: gravity, motor_gain and motor_strength are all NULL"); return RP_ERR_ARG; }
  const int na = h->host_model.n_arm;
  return table_get(h, h->act, {gravity, motor_gain, motor_strength, 3, na, na}, stream);
}

/* enqueued on `stream` like rp_set_wrench; writes the named words of the state records (and, with RP_KIN_CLEAR_CONTACTS, zeroes the cache rows) and nothing else */
int rp_set_kinematics(rp_handle h, const float* pos, const float* vel, int32_t rows, const uint8_t* mask, uint32_t flags, void* stream) {
  if (!h) return RP_ERR_ARG;
  const int N = h->cfg.num_envs, na = h->host_model.n_arm, nf = h->host_model.n_free, nj = h->host_model.n_j1;
  if (!pos && !vel) { snprintf(h->err, 256, "rp_set_kinematics: pos and vel are both NULL"); return RP_ERR_ARG; }
  if (!rows_ok(h, "rp_set_kinematics", rows)) return RP_ERR_ARG;
  if (flags & ~(uint32_t)RP_KIN_CLEAR_CONTACTS) { snprintf(h->err, 256, "rp_set_kinematics: unknown bits in flags (0x%x)", flags); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  const int nclr = (flags & RP_KIN_CLEAR_CONTACTS) && h->pmcache ? PMC_FLOATS : 0;
  const size_t total = (size_t)N * (2 * na + 13 * nf + 2 * nj + nclr);
  hipLaunchKernelGGL(k_set_kinematics, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->state, h->pmcache, pos, vel, (int)rows, mask, N, na, nf,
                     nj, nclr);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_get_kinematics(rp_handle h, float* pos, float* vel, void* stream) {
  if (!h || (!pos && !vel)) { if (h) snprintf(h->err, 256, "rp_get_kinematics: pos and vel are both NULL"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs, na = h->host_model.n_arm, nf = h->host_model.n_free, nj = h->host_model.n_j1;
  const size_t total = (size_t)N * (2 * na + 13 * nf + 2 * nj);
  hipLaunchKernelGGL(k_get_kinematics, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)h->state, pos, vel, N, na, nf, nj);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_get_visuals_dims(rp_handle h, int32_t* n_col) {
  if (!h || !n_col) return RP_ERR_ARG;
  *n_col = h->host_model.n_col;
  return RP_OK;
}

/* the visuals table at its first use: up to 800 B per env (2.7 GB at the 4 M envs rp_create allows), so a handle that never randomises its image never pays for it.
 * Allocated here, as rp_copy_envs allocates its staging buffer, and every env's row filled with the default one through launch_table_set on `stream`, ahead of the
 * caller's set or get: the colours straight from the device model's col_rgb (what k_collider_poses reads without a table), the light and the background - rp_render.cuh's
 * literals - from eight words behind the table, written on the same stream.  Nothing waits on the host and no device value is read. */
static int vis_reserve(rp_sim* h, void* stream) {
  if (h->vis) return RP_OK;
  const int nc = h->host_model.n_col, W = 3 * nc + VIS_TAIL;
  const size_t N = (size_t)h->cfg.num_envs;
  const float tail[VIS_TAIL] = {VIS_LIGHT_X, VIS_LIGHT_Y, VIS_LIGHT_Z, VIS_AMBIENT, VIS_DIFFUSE, VIS_BG_R, VIS_BG_G, VIS_BG_B};
  float* tab = nullptr;
  HIPCHK(h, hipMalloc((void**)&tab, (N * W + VIS_TAIL) * sizeof(float)));
  float* base = tab + N * W;
  hipError_t e = hipSuccess;
  for (int k = 0; k < VIS_TAIL && e == hipSuccess; k++) {
    int word;
    memcpy(&word, &tail[k], sizeof(word));
    e = hipMemsetD32Async((hipDeviceptr_t)(base + k), word, 1, (hipStream_t)stream);
  }
  if (e == hipSuccess) {
    launch_table_set(h, tab, {&h->dev_model->col_rgb[0][0], base, base + 5, 3 * nc, 5, 3}, 0, 1, nullptr, stream);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { hipFree(tab); snprintf(h->err, 256, "rp_set_visuals / rp_get_visuals: the table's default rows: %s", hipGetErrorString(e)); return RP_ERR_HIP; }
  h->vis = tab;
  return RP_OK;
}

/* enqueued on `stream` like rp_set_dynamics: a render queued after it on the same stream draws with the new values, one queued before it with the old ones */
int rp_set_visuals(rp_handle h, const float* colour, const float* light, const float* background, int32_t rows, const uint8_t* mask, void* stream) {
  if (!h) return RP_ERR_ARG;
  if (!colour && !light && !background) { snprintf(h->err, 256, "rp_set_visuals: colour, light and background are all NULL"); return RP_ERR_ARG; }
  if (!rows_ok(h, "rp_set_visuals", rows)) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  int rc = vis_reserve(h, stream);
  if (rc != RP_OK) return rc;
  return table_set(h, "rp_set_visuals", h->vis, {colour, light, background, 3 * h->host_model.n_col, 5, 3}, 0, rows, mask, stream);
}

int rp_get_visuals(rp_handle h, float* colour, float* light, float* background, void* stream) {
  if (!h || (!colour && !light && !background)) { if (h) snprintf(h->err, 256, "rp_get_visuals: colour, light and background are all NULL"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  int rc = vis_reserve(h, stream);
  if (rc != RP_OK) return rc;
  return table_get(h, h->vis, {colour, light, background, 3 * h->host_model.n_col, 5, 3}, stream);
}

/* two launches on `stream`: every row into the handle's staging buffer, then the masked envs' rows out of it (k_copy_envs_stage / k_copy_envs_gather) */
int rp_copy_envs(rp_handle h, const int32_t* src, const uint8_t* mask, uint32_t flags, void* stream) {
  if (!h) return RP_ERR_ARG;
  if (!src) { snprintf(h->err, 256, "rp_copy_envs: src is NULL"); return RP_ERR_ARG; }
  if (flags & ~(uint32_t)RP_COPY_EPISODE_STEPS) { snprintf(h->err, 256, "rp_copy_envs: unknown bits in flags (0x%x)", flags); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs, nc4 = h->pmcache ? PMC_FLOATS / 4 : 0;
  const size_t W = RP_REC_FLOATS / 4 + (size_t)nc4, total = (size_t)N * W;
  if (!h->cp_stage) HIPCHK(h, hipMalloc((void**)&h->cp_stage, total * sizeof(float4) + (size_t)N * sizeof(int)));
  float4* stage = (float4*)h->cp_stage;
  int* steps_stage = (int*)(stage + total);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_copy_envs_stage, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, stage, steps_stage, (const float4*)h->state, (const float4*)h->pmcache,
                     (const int*)h->ep_steps, N, nc4);
  hipLaunchKernelGGL(k_copy_envs_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (float4*)h->state, (float4*)h->pmcache, h->ep_steps, (const float4*)stage,
                     (const int*)steps_stage, (const int*)src, mask, N, nc4, (flags & RP_COPY_EPISODE_STEPS) ? 1 : 0);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_get_reset_rows(rp_handle h, int32_t* dst, void* stream) {
  if (!h || !dst) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  HIPCHK(h, hipMemcpyAsync(dst, h->rt_env_row, (size_t)h->cfg.num_envs * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RP_OK;
}

int rp_calc_state(rp_handle h, const rp_out* out, void* stream) {
  if (!h) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  int N = h->cfg.num_envs;
  hipLaunchKernelGGL(k_calc_state, dim3(N), dim3(64), 0, (hipStream_t)stream, h->dev_model, h->state, to_ptrs(out), 0, N, (const int*)nullptr);
  image_pass(h, false, nullptr, nullptr, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

static int reward_impl(rp_handle h, const float* ag, const float* dg, float* r, int32_t m, void* stream, int force_sparse) {
  if (!h || !ag || !dg || !r || m < 0) return RP_ERR_ARG;
  if (m == 0) return RP_OK;
  DevGuard guard(h->cfg.device);
  hipLaunchKernelGGL(k_reward, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dev_model, ag, dg, r, m, force_sparse);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}
int rp_compute_reward(rp_handle h, const float* ag, const float* dg, float* r, int32_t m, void* stream) { return reward_impl(h, ag, dg, r, m, stream, 0); }
int rp_compute_reward_sparse(rp_handle h, const float* ag, const float* dg, float* r, int32_t m, void* stream) { return reward_impl(h, ag, dg, r, m, stream, 1); }

size_t rp_state_bytes(rp_handle h) { return (RP_REC_FLOATS + (h && h->pmcache ? PMC_FLOATS : 0)) * sizeof(float); }

int rp_get_state(rp_handle h, void* dst, void* stream) {
  if (!h || !dst) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs, nc = h->pmcache ? PMC_FLOATS : 0;
  const size_t total = (size_t)N * (RP_REC_FLOATS + nc);
  hipLaunchKernelGGL(k_read_state, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float*)dst, h->state, h->pmcache, N, nc);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_set_state(rp_handle h, const void* src, int32_t src_env_count, void* stream) {
  if (!h || !src) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  int N = h->cfg.num_envs;
  if (src_env_count != 1 && src_env_count != N) { snprintf(h->err, 256, "rp_set_state: src_env_count %d is neither 1 nor %d", src_env_count, N); return RP_ERR_STATE_SIZE; }
  const int nc = h->pmcache ? PMC_FLOATS : 0;
  const size_t total = (size_t)N * (RP_REC_FLOATS + nc);
  hipLaunchKernelGGL(k_copy_state, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->state, h->pmcache, (const float*)src, N, src_env_count, nc);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_set_debug_flags(rp_handle h, int32_t flags) { if (!h) return RP_ERR_ARG; h->debug_flags = flags & 1; return RP_OK; }   /* bit 1 is internal (k_action_prep) */
int rp_set_groups(rp_handle h, int32_t groups) { if (!h || groups < 1 || groups > RP_MAX_GROUPS) return RP_ERR_ARG; h->groups = groups; return RP_OK; }
int rp_set_fused(rp_handle h, int32_t fused) {
  if (!h || fused < 0 || fused > 2) return RP_ERR_ARG;
  if (fused == 2 && h->timers_on) { snprintf(h->err, 256, "rp_set_fused: the k_chain pipeline has no per-launch timers (rp_enable_timers(h, 0) first)"); return RP_ERR_ARG; }
  if (fused != h->fused) h->sort_G = 0;          /* the load tables of one pipeline mean nothing to the other: start from the identity ranking */
  h->fused = fused;
  return RP_OK;
}
static int rc_reserve(rp_handle h, int num) {
  if (num <= h->rc_cap) return RP_OK;
  hipFree(h->rc_tab); hipFree(h->rc_cnt); hipFree(h->rc_ee);
  h->rc_tab = nullptr; h->rc_cnt = nullptr; h->rc_ee = nullptr; h->rc_cap = 0;
  HIPCHK(h, hipMalloc((void**)&h->rc_tab, (size_t)num * RC_MAX * RC_STRIDE * sizeof(float)));
  HIPCHK(h, hipMalloc((void**)&h->rc_cnt, (size_t)num * sizeof(int)));
  HIPCHK(h, hipMalloc((void**)&h->rc_ee, (size_t)num * 20 * sizeof(float)));      /* [num][12] EE poses, then [num][8] the ghost arm's joints of the latest rp_render_ex (rp_debug_ghost_joints) */
  h->rc_cap = num;
  return RP_OK;
}

int rp_camera_from_yaw_pitch_roll(const float target[3], float distance, float yaw_deg, float pitch_deg, float roll_deg, rp_camera* cam) {
  if (!target || !cam) return RP_ERR_ARG;
  /* b3ComputeViewMatrixFromYawPitchRoll, upAxis 2: eye = target + R (0, -distance, 0), up = R (0, 0, 1), R = Rz(yaw) Ry(roll) Rx(pitch) */
  const double d2r = 0.01745329251994329547, y = yaw_deg * d2r, p = pitch_deg * d2r, r = roll_deg * d2r;
  const double cy = cos(y), sy = sin(y), cp = cos(p), sp = sin(p), cr = cos(r), sr = sin(r);
  const double R[9] = {cy * cr, cy * sr * sp - sy * cp, cy * sr * cp + sy * sp, sy * cr, sy * sr * sp + cy * cp, sy * sr * cp - cy * sp, -sr, cr * sp, cr * cp};
  memset(cam, 0, sizeof(*cam));
  for (int k = 0; k < 3; k++) { cam->target[k] = target[k]; cam->eye[k] = target[k] + (float)(R[3 * k + 1] * -distance); cam->up[k] = (float)R[3 * k + 2]; }
  cam->fov_deg = 50.f; cam->aspect = 1.f; cam->mode = 0;
  return RP_OK;
}
int rp_default_camera(rp_camera* cam) {
  const float target[3] = {0.f, 0.25f, 0.f};
  return rp_camera_from_yaw_pitch_roll(target, 1.3f, -30.f, -30.f, 0.f, cam);
}

static RpCamera device_camera(const rp_camera* c) {
  RpCamera d; memset(&d, 0, sizeof(d));
  double f[3], u[3], s[3], n = 0;
  for (int k = 0; k < 3; k++) { f[k] = c->target[k] - c->eye[k]; n += f[k] * f[k]; }
  n = sqrt(n > 0 ? n : 1);
  for (int k = 0; k < 3; k++) f[k] /= n;
  s[0] = f[1] * c->up[2] - f[2] * c->up[1]; s[1] = f[2] * c->up[0] - f[0] * c->up[2]; s[2] = f[0] * c->up[1] - f[1] * c->up[0];
  n = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); n = n > 0 ? n : 1;
  for (int k = 0; k < 3; k++) s[k] /= n;
  u[0] = s[1] * f[2] - s[2] * f[1]; u[1] = s[2] * f[0] - s[0] * f[2]; u[2] = s[0] * f[1] - s[1] * f[0];
  for (int k = 0; k < 3; k++) { d.eye[k] = c->eye[k]; d.fwd[k] = (float)f[k]; d.right[k] = (float)s[k]; d.up[k] = (float)u[k]; }
  d.tan_half_fov = (float)tan(0.5 * c->fov_deg * 0.01745329251994329547); d.aspect = c->aspect; d.mode = c->mode;
  return d;
}

/* the checks of a draw (`who` names the entry point in the messages): the size and range checks, the Panda-only ghost arm, the tile-count limit, the camera (NULL and
 * no cam_rows = the default one); *e gets the camera, the size with its tile counts and the depth mapping - the outputs and tile0 stay zero for the caller.  Touches
 * no device. */
static int views_check(rp_handle h, const char* who, const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane, int metres, int32_t width,
                       int32_t height, int32_t first_env, int32_t num_envs, const float* ghost_arm, RpViewEntry* e) {
  const char* bad = nullptr;
  if (width <= 0 || height <= 0 || width > 4096 || height > 4096) bad = "bad image size";
  else if (first_env < 0 || num_envs <= 0 || first_env + num_envs > h->cfg.num_envs) bad = "bad env range";
  if (bad) { snprintf(h->err, 256, "%s: %s", who, bad); return RP_ERR_ARG; }
  if (ghost_arm && h->host_model.arm_type != RP_ARM_PANDA) {      /* environments.py:629-630: the reference has a ghost arm for the Panda only and raises for the UR5 */
    snprintf(h->err, 256, "%s: the ghost arm exists for the Panda only (environments.py:623-630)", who); return RP_ERR_UNSUPPORTED;
  }
  const long long blocks = (long long)num_envs * ((width + 15) / 16) * ((height + 15) / 16);
  if (blocks > 0x7fffffffLL) { snprintf(h->err, 256, "%s: %lld tiles exceed one launch", who, blocks); return RP_ERR_ARG; }
  rp_camera def;
  memset(e, 0, sizeof(*e));
  if (!cam_rows) {
    if (!cam) { rp_default_camera(&def); cam = &def; }
    if (cam->mode < 0 || cam->mode > 1 || !(cam->fov_deg > 0.f && cam->fov_deg < 180.f) || !(cam->aspect > 0.f)) { snprintf(h->err, 256, "%s: bad camera", who); return RP_ERR_ARG; }
    e->cam = device_camera(cam);
  }
  e->cam_rows = cam_rows; e->near_plane = near_plane; e->far_plane = far_plane; e->metres = metres;
  e->width = width; e->height = height; e->tiles_x = (width + 15) / 16; e->tiles = e->tiles_x * ((height + 15) / 16);
  return RP_OK;
}

/* THE k_collider_poses launch: the pose table of envs [first, first + num) on `s` (rc_reserve has made room for num), with the selection sel32 / sel8 (rc_selected;
 * indexed by env, so a selection goes with first = 0).  The kernels' SEL = true instantiations only where there is a selection: without one they are the kernels they
 * were.  ee: where the EE poses go (h->rc_ee; null: nobody reads them), vis: the visuals table (h->vis, null until the first rp_set_visuals / rp_get_visuals). */
static void poses_launch(rp_sim* h, int first, int num, const float* sub_goal, float* ee, const float* ghost_arm, const float* vis, const int32_t* sel32,
                         const uint8_t* sel8, hipStream_t s) {
  hipLaunchKernelGGL((sel32 || sel8) ? k_collider_poses<true> : k_collider_poses<false>, dim3(num), dim3(64), 0, s, h->dev_model, h->state, first, num, h->rc_tab, h->rc_cnt,
                     sub_goal, ee, ghost_arm, vis, (const int*)sel32, sel8);
}

/* THE k_render_layers launch: entry e (views_check, with the caller's outputs) for the `num` envs of the pose table, which are envs [first, first + num) */
static void layers_launch(rp_sim* h, const RpViewEntry& e, int first, int num, const int32_t* sel32, const uint8_t* sel8, hipStream_t s) {
  hipLaunchKernelGGL((sel32 || sel8) ? k_render_layers<true> : k_render_layers<false>, dim3((unsigned)num * (unsigned)e.tiles), dim3(256), 0, s, h->dev_model, h->rc_tab,
                     h->rc_cnt, num, e.cam, e.cam_rows, h->rc_ee, e.width, e.height, h->render_nocull ? 0 : 1, e.near_plane, e.far_plane, e.metres, e.rgb, e.depth, e.seg,
                     (const float*)h->vis, first, (const int*)sel32, sel8);
}

/* The image configuration's draw inside a call that writes observation rows: all N envs, or those sel32 / sel8 select on the device, into the observation tensors
 * (final = false) or the ended envs' (final = true: rp_step_autoreset's terminal pass).  ONE k_collider_poses over all N envs - the poses and rc_ee do not depend on
 * the camera -, then a configuration of one view draws its entry with k_render_layers and one of several draws the pass's entries with ONE k_render_views, whose grid
 * holds the tiles of them all (the choice is by the configuration's views, not the pass's); with rp_debug_image_views_merge(h, 0) a k_render_layers launch per entry
 * instead.  Same bytes.  Nothing is checked, reserved or read back here. */
static void image_pass(rp_sim* h, bool final, const int32_t* sel32, const uint8_t* sel8, hipStream_t s) {
  const RpImageConfig& c = h->img;
  if (!c.n || (final && !c.n_fin)) return;
  const RpViewTable& t = final ? c.fin : c.obs;
  const int n = final ? c.n_fin : c.n, tiles = final ? c.ftiles : c.tiles, N = h->cfg.num_envs;
  poses_launch(h, 0, N, nullptr, h->rc_ee, nullptr, h->vis, sel32, sel8, s);
  if (c.n == 1 || h->iv_nomerge)
    for (int k = 0; k < n; k++) layers_launch(h, t.v[k], 0, N, sel32, sel8, s);
  else
    hipLaunchKernelGGL((sel32 || sel8) ? k_render_views<true> : k_render_views<false>, dim3((unsigned)N * (unsigned)tiles), dim3(256), 0, s, h->dev_model, h->rc_tab, h->rc_cnt, N,
                       t, n, tiles, h->rc_ee, h->render_nocull ? 0 : 1, (const float*)h->vis, (const int*)sel32, sel8);
  if (c.pc_n) points_pass(h, final, sel32, sel8, s);
}

/* k_point_cloud for `n` table entries over envs [first_env, first_env + num) on `s`, behind the draw that wrote their layers (and rc_ee, which the gripper camera's
 * basis reads) */
static void points_launch(rp_sim* h, const RpPointsTable& t, int n, int first_env, int num, const int32_t* sel32, const uint8_t* sel8, hipStream_t s) {
  const bool sel = sel32 || sel8;
  hipLaunchKernelGGL(sel ? k_point_cloud<true> : k_point_cloud<false>, dim3((unsigned)n * (unsigned)num), dim3(256), 0, s, t, n, num, first_env, (const float*)h->rc_ee,
                     (const int*)sel32, sel8);
}

/* rp_set_image_points' launch behind an image pass: ONE k_point_cloud for all views of the pass that have a cloud, with the pass's selection */
static void points_pass(rp_sim* h, bool final, const int32_t* sel32, const uint8_t* sel8, hipStream_t s) {
  RpPointsTable t;
  int n = 0;
  for (int k = 0; k < RC_MAX_VIEWS; k++)
    if (h->img.pc_has[k] & (final ? 2 : 1)) t.v[n++] = final ? h->img.pc_fin[k] : h->img.pc_obs[k];
  for (int k = n; k < RC_MAX_VIEWS; k++) memset(&t.v[k], 0, sizeof(t.v[k]));
  if (n) points_launch(h, t, n, 0, h->cfg.num_envs, sel32, sel8, s);
}

/* every attachment goes with the image configuration it was made on (rp_set_image_obs, rp_set_image_views: replaced or switched off) */
static void points_drop(rp_sim* h) { h->img.pc_n = 0; memset(h->img.pc_has, 0, sizeof(h->img.pc_has)); }

/* rp_points_spec's own rules: the complaint, or null */
static const char* spec_complaint(const rp_points_spec* spec) {
  if (!spec) return "spec is NULL";
  if (spec->max_points < 1 || spec->max_points > 65536) return "max_points lies outside 1 .. 65536";
  if (spec->frame != RP_POINTS_WORLD && spec->frame != RP_POINTS_CAMERA) return "unknown frame";
  if (!(spec->max_depth == spec->max_depth)) return "max_depth is not a number";
  return nullptr;
}

/* a draw of an entry point: the pose table for envs [first_env, first_env + num_envs), then entry e (views_check, with the caller's outputs), on `stream` */
static int entry_draw(rp_handle h, const RpViewEntry& e, int32_t first_env, int32_t num_envs, const float* sub_goal, const float* ghost_arm, void* stream) {
  int rc = rc_reserve(h, num_envs);
  if (rc != RP_OK) return rc;
  h->rc_last_num = num_envs;
  poses_launch(h, first_env, num_envs, sub_goal, h->rc_ee, ghost_arm, h->vis, nullptr, nullptr, (hipStream_t)stream);
  layers_launch(h, e, first_env, num_envs, nullptr, nullptr, (hipStream_t)stream);
  return RP_OK;
}

/* the one path behind rp_render_ex and rp_render_layers: views_check, entry_draw */
static int render_views(rp_handle h, const char* who, const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane, int metres, int32_t width,
                        int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb, float* depth, int32_t* segmentation, const float* sub_goal,
                        const float* ghost_arm, void* stream) {
  RpViewEntry e;
  int rc = views_check(h, who, cam, cam_rows, near_plane, far_plane, metres, width, height, first_env, num_envs, ghost_arm, &e);
  if (rc != RP_OK) return rc;
  e.rgb = rgb; e.depth = depth; e.seg = segmentation;
  DevGuard guard(h->cfg.device);
  rc = entry_draw(h, e, first_env, num_envs, sub_goal, ghost_arm, stream);
  if (rc != RP_OK) return rc;
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

/* rp_render_layers' own argument rules, which rp_set_image_obs shares: the complaint, or null */
static const char* layers_complaint(const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane, int32_t depth_mode, const void* rgb, const void* depth,
                                    const void* segmentation) {
  if (!rgb && !depth && !segmentation) return "no output layer (rgb, depth and segmentation are all NULL)";
  if (cam && cam_rows) return "both cam and cam_rows given";
  if (!(near_plane > 0.f)) return "near_plane <= 0";
  if (!(far_plane > near_plane)) return "far_plane <= near_plane";
  if (depth_mode != RP_DEPTH_BUFFER && depth_mode != RP_DEPTH_METRES) return "unknown depth mode";
  return nullptr;
}

/* The image configuration: every check is made here, once, and the stepping calls only launch (image_pass).  `who` is the entry point; with `numbered` a complaint
 * about view k names it ("<who>: view k: ...").  Every view is checked before anything changes: a refusal leaves the configuration in force as it was.  n = 0
 * switches it off.  The pose table is reserved for all N envs here, so that no stepping call allocates; where that replaces a smaller table, hipFree waits for the
 * device, and so does this call before it replaces a configuration that calls in flight on other streams were launched with (their kernels hold the old pointers;
 * the caller may free those buffers once this call has returned). */
static int image_config_set(rp_handle h, const char* who, bool numbered, const rp_image_view* views, int n) {
  const int N = h->cfg.num_envs;
  RpImageConfig c;
  memset(&c, 0, sizeof(c));
  for (int k = 0; k < RC_MAX_VIEWS; k++) c.fmap[k] = -1;
  long long tiles = 0, ftiles = 0;
  for (int k = 0; k < n; k++) {
    const rp_image_view& w = views[k];
    char name[48];
    if (numbered) snprintf(name, sizeof(name), "%s: view %d", who, k);
    else snprintf(name, sizeof(name), "%s", who);
    const char* bad = layers_complaint(w.cam, w.cam_rows, w.near_plane, w.far_plane, w.depth_mode, w.rgb, w.depth, w.segmentation);
    if (bad) { snprintf(h->err, 256, "%s: %s", name, bad); return RP_ERR_ARG; }
    RpViewEntry e;
    int rc = views_check(h, name, w.cam, w.cam_rows, w.near_plane, w.far_plane, w.depth_mode == RP_DEPTH_METRES ? 1 : 0, w.width, w.height, 0, N, nullptr, &e);
    if (rc != RP_OK) return rc;
    e.tile0 = (int)tiles; e.rgb = w.rgb; e.depth = w.depth; e.seg = w.segmentation;
    c.obs.v[k] = e;
    tiles += e.tiles;
    /* a terminal layer without its observation layer is drawn all the same: the final_* pointers stand for themselves */
    if (w.final_rgb || w.final_depth || w.final_segmentation) {
      e.tile0 = (int)ftiles; e.rgb = w.final_rgb; e.depth = w.final_depth; e.seg = w.final_segmentation;
      c.fmap[k] = c.n_fin;
      c.fin.v[c.n_fin++] = e;
      ftiles += e.tiles;
    }
  }
  if ((long long)N * tiles > 0x7fffffffLL) { snprintf(h->err, 256, "%s: %lld tiles of %d views exceed one launch", who, (long long)N * tiles, n); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  if (h->img.n) HIPCHK(h, hipDeviceSynchronize());
  h->img.n = 0;      /* (off until the pose table stands: a failed reserve may have freed the one it had) */
  points_drop(h);    /* rp_set_image_points' clouds go with the configuration they were attached to */
  if (n == 0) return RP_OK;
  int rc = rc_reserve(h, N);
  if (rc != RP_OK) return rc;
  c.n = n; c.tiles = (int)tiles; c.ftiles = (int)ftiles;
  h->img = c;
  return RP_OK;
}

int rp_set_image_obs(rp_handle h, const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane, int32_t depth_mode, int32_t width, int32_t height,
                     uint8_t* rgb, float* depth, int32_t* segmentation, uint8_t* final_rgb, float* final_depth, int32_t* final_segmentation) {
  if (!h) return RP_ERR_ARG;
  rp_image_view w;
  memset(&w, 0, sizeof(w));
  w.cam = cam; w.cam_rows = cam_rows; w.near_plane = near_plane; w.far_plane = far_plane; w.depth_mode = depth_mode; w.width = width; w.height = height;
  w.rgb = rgb; w.depth = depth; w.segmentation = segmentation; w.final_rgb = final_rgb; w.final_depth = final_depth; w.final_segmentation = final_segmentation;
  return image_config_set(h, "rp_set_image_obs", false, &w, width == 0 && height == 0 ? 0 : 1);
}

/* Several views per env: the same configuration with up to RP_MAX_IMAGE_VIEWS entries */
int rp_set_image_views(rp_handle h, const rp_image_view* views, int32_t n_views) {
  if (!h) return RP_ERR_ARG;
  if (n_views < 0 || n_views > RP_MAX_IMAGE_VIEWS) { snprintf(h->err, 256, "rp_set_image_views: n_views = %d lies outside 0 .. %d", n_views, RP_MAX_IMAGE_VIEWS); return RP_ERR_ARG; }
  if (n_views > 0 && !views) { snprintf(h->err, 256, "rp_set_image_views: views is NULL with n_views = %d", n_views); return RP_ERR_ARG; }
  return image_config_set(h, "rp_set_image_views", true, views, n_views);
}

/* test seam and benchmark control: on = 0 draws the views of a pass as one k_render_layers launch each (the default is on: one k_render_views launch) */
int rp_debug_image_views_merge(rp_handle h, int32_t on) { if (!h) return RP_ERR_ARG; h->iv_nomerge = on ? 0 : 1; return RP_OK; }

int rp_render_ex(rp_handle h, const rp_camera* cam, int32_t width, int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb,
                 const float* sub_goal, const float* ghost_arm, void* stream) {
  if (!h) return RP_ERR_ARG;
  if (!rgb) { snprintf(h->err, 256, "rp_render_ex: no output image (rgb is NULL)"); return RP_ERR_ARG; }
  return render_views(h, "rp_render_ex", cam, nullptr, 0.01f, 10.f, 0, width, height, first_env, num_envs, rgb, nullptr, nullptr, sub_goal, ghost_arm, stream);      /* (near, far and the mode shape the depth value only) */
}

int rp_render(rp_handle h, const rp_camera* cam, int32_t width, int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb,
              const float* sub_goal, void* stream) {
  return rp_render_ex(h, cam, width, height, first_env, num_envs, rgb, sub_goal, nullptr, stream);
}

int rp_render_layers(rp_handle h, const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane, int32_t depth_mode,
                     int32_t width, int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb, float* depth, int32_t* segmentation,
                     const float* sub_goal, const float* ghost_arm, void* stream) {
  if (!h) return RP_ERR_ARG;
  const char* bad = layers_complaint(cam, cam_rows, near_plane, far_plane, depth_mode, rgb, depth, segmentation);
  if (bad) { snprintf(h->err, 256, "rp_render_layers: %s", bad); return RP_ERR_ARG; }
  return render_views(h, "rp_render_layers", cam, cam_rows, near_plane, far_plane, depth_mode == RP_DEPTH_METRES ? 1 : 0, width, height, first_env, num_envs, rgb, depth,
                      segmentation, sub_goal, ghost_arm, stream);
}

/* Images of state rows that need not be the handle's own: per chunk of images k_collider_poses_rows and k_render_states on `stream`, every pointer moved to the chunk's
 * first image on the host.  A chunk holds min(m, max(N, 4096)) images (rp_debug_render_states_chunk: a test's cap), fewer where its tiles would exceed one launch.
 * Only the pose table is written (and grown, by rc_reserve, to the chunk size): h->state is read where src->rows is NULL and nothing else of the handle is touched. */
int rp_render_states(rp_handle h, const rp_state_rows* src, int32_t m, const rp_camera* cam, const float* cam_rows, float near_plane, float far_plane,
                     int32_t depth_mode, int32_t width, int32_t height, uint8_t* rgb, float* depth, int32_t* segmentation, const float* goal, int32_t goal_mode,
                     void* stream) {
  if (!h) return RP_ERR_ARG;
  const int N = h->cfg.num_envs;
  const char* bad = nullptr;
  if (!src) bad = "src is NULL";
  else if (m < 1) bad = "m < 1";
  else if (src->rows && src->row_stride < RP_REC_FLOATS * sizeof(float)) bad = "row_stride < 512";
  else if (src->rows && src->row_stride % 4 != 0) bad = "row_stride is not a multiple of 4";
  else if (src->rows && src->n_rows < 1) bad = "n_rows < 1";
  else if (!src->row_index && m > (src->rows ? src->n_rows : N)) bad = src->rows ? "m exceeds n_rows and row_index is NULL" : "m exceeds the handle's envs and row_index is NULL (live rows)";
  else if (goal_mode != RP_GOAL_GHOST && goal_mode != RP_GOAL_SOLID) bad = "unknown goal_mode";
  if (!bad) bad = layers_complaint(cam, cam_rows, near_plane, far_plane, depth_mode, rgb, depth, segmentation);
  if (bad) { snprintf(h->err, 256, "rp_render_states: %s", bad); return RP_ERR_ARG; }
  RpViewEntry e;
  int rc = views_check(h, "rp_render_states", cam, cam_rows, near_plane, far_plane, depth_mode == RP_DEPTH_METRES ? 1 : 0, width, height, 0, 1, nullptr, &e);
  if (rc != RP_OK) return rc;
  const float* rows = src->rows ? (const float*)src->rows : h->state;
  const size_t row_floats = src->rows ? src->row_stride / sizeof(float) : (size_t)RP_REC_FLOATS;
  const int n_rows = src->rows ? src->n_rows : N;
  const long long tiles = e.tiles;       /* <= 65536: a chunk never falls below 32767 images */
  long long cap = h->rs_chunk > 0 ? h->rs_chunk : (N > 4096 ? N : 4096);
  if (cap > m) cap = m;
  if (cap * tiles > 0x7fffffffLL) cap = 0x7fffffffLL / tiles;
  DevGuard guard(h->cfg.device);
  rc = rc_reserve(h, (int)cap);
  if (rc != RP_OK) return rc;
  const size_t npix = (size_t)width * height;
  const int n_ag = h->host_model.n_ag, cull = h->render_nocull ? 0 : 1;
  hipStream_t s = (hipStream_t)stream;
  for (long long base = 0; base < m; base += cap) {
    const int num = (int)(m - base < cap ? m - base : cap);
    const int* idx = src->row_index ? src->row_index + base : nullptr;
    const int* ve = src->vis_env ? src->vis_env + base : nullptr;
    const float* g = goal ? goal + (size_t)base * n_ag : nullptr;
    hipLaunchKernelGGL(goal_mode == RP_GOAL_SOLID ? k_collider_poses_rows<true> : k_collider_poses_rows<false>, dim3(num), dim3(64), 0, s, h->dev_model, rows, row_floats,
                       n_rows, idx, (int)base, num, h->rc_tab, h->rc_cnt, g, h->rc_ee, (const float*)h->vis, ve, N);
    hipLaunchKernelGGL(k_render_states, dim3((unsigned)(num * tiles)), dim3(256), 0, s, h->dev_model, h->rc_tab, h->rc_cnt, num, e.cam,
                       cam_rows ? cam_rows + 11 * (size_t)base : nullptr, h->rc_ee, width, height, cull, near_plane, far_plane, e.metres,
                       rgb ? rgb + 3 * npix * (size_t)base : nullptr, depth ? depth + npix * (size_t)base : nullptr,
                       segmentation ? segmentation + npix * (size_t)base : nullptr, (const float*)h->vis, ve, N, idx, (int)base, n_rows);
  }
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

/* test seam: the most images one chunk of rp_render_states holds (0 = the rule: min(m, max(N, 4096))) */
int rp_debug_render_states_chunk(rp_handle h, int32_t slots) {
  if (!h || slots < 0) return RP_ERR_ARG;
  h->rs_chunk = slots;
  return RP_OK;
}

/* one table entry: the camera, the size and the layers of view entry v (the layers to read), the spec, the outputs */
static RpPointsEntry points_entry(const RpViewEntry& v, const rp_points_spec* spec, float* xyz, int32_t* point_seg, uint8_t* point_rgb, int32_t* count) {
  RpPointsEntry e;
  memset(&e, 0, sizeof(e));
  e.cam = v.cam; e.cam_rows = v.cam_rows; e.width = v.width; e.height = v.height;
  e.depth = v.depth; e.seg = v.seg; e.rgb = point_rgb ? v.rgb : nullptr;
  e.xyz = xyz; e.pseg = point_seg; e.prgb = point_rgb; e.count = count;
  e.max_points = spec->max_points; e.frame = spec->frame; e.max_depth = spec->max_depth; e.drop = spec->drop;
  return e;
}

/* Point clouds behind a draw of its own: k_collider_poses, k_render_layers (metres, near 0.01, far 10, no ghosts, the handle's visuals) into the caller's layer
 * buffers, k_point_cloud - three launches on `stream`, nothing read back. */
int rp_render_points(rp_handle h, const rp_camera* cam, const float* cam_rows, int32_t width, int32_t height, int32_t first_env, int32_t num_envs,
                     const rp_points_spec* spec, uint8_t* rgb, float* depth, int32_t* segmentation, float* xyz, int32_t* point_seg, uint8_t* point_rgb,
                     int32_t* count, void* stream) {
  if (!h) return RP_ERR_ARG;
  const char* bad = spec_complaint(spec);
  if (!bad && (!depth || !segmentation)) bad = "the depth and segmentation layer buffers are both required";
  if (!bad && !xyz && !count) bad = "no output (xyz and count are both NULL)";
  if (!bad && point_rgb && !rgb) bad = "point_rgb needs the rgb layer buffer";
  if (!bad) bad = layers_complaint(cam, cam_rows, 0.01f, 10.f, RP_DEPTH_METRES, rgb, depth, segmentation);
  if (bad) { snprintf(h->err, 256, "rp_render_points: %s", bad); return RP_ERR_ARG; }
  RpViewEntry e;
  int rc = views_check(h, "rp_render_points", cam, cam_rows, 0.01f, 10.f, 1, width, height, first_env, num_envs, nullptr, &e);
  if (rc != RP_OK) return rc;
  e.rgb = rgb; e.depth = depth; e.seg = segmentation;
  DevGuard guard(h->cfg.device);
  rc = entry_draw(h, e, first_env, num_envs, nullptr, nullptr, stream);
  if (rc != RP_OK) return rc;
  RpPointsTable t;
  memset(&t, 0, sizeof(t));
  t.v[0] = points_entry(e, spec, xyz, point_seg, point_rgb, count);
  points_launch(h, t, 1, first_env, num_envs, nullptr, nullptr, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

/* A cloud on view `view` of the image configuration in force: every check is made here, a stepping call only launches (points_pass).  A refusal leaves the
 * attachments as they were. */
int rp_set_image_points(rp_handle h, int32_t view, const rp_points_spec* spec, float* xyz, int32_t* point_seg, uint8_t* point_rgb, int32_t* count, float* final_xyz,
                        int32_t* final_point_seg, uint8_t* final_point_rgb, int32_t* final_count) {
  if (!h) return RP_ERR_ARG;
  RpImageConfig& c = h->img;
  if (!c.n) { snprintf(h->err, 256, "rp_set_image_points: no image configuration is in force (rp_set_image_obs or rp_set_image_views first)"); return RP_ERR_ARG; }
  if (view < 0 || view >= c.n) { snprintf(h->err, 256, "rp_set_image_points: view %d lies outside 0 .. %d", view, c.n - 1); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  if (!spec) {      /* detach: calls in flight may still write the old outputs */
    if (c.pc_has[view]) { HIPCHK(h, hipDeviceSynchronize()); c.pc_has[view] = 0; c.pc_n--; }
    return RP_OK;
  }
  /* the view's entries, observation and terminal (without one: no terminal layers) */
  const RpViewEntry& e = c.obs.v[view];
  RpViewEntry f;
  memset(&f, 0, sizeof(f));
  if (c.fmap[view] >= 0) f = c.fin.v[c.fmap[view]];
  const bool fin = final_xyz || final_point_seg || final_point_rgb || final_count;
  const char* bad = spec_complaint(spec);
  if (!bad && (!e.depth || !e.metres)) bad = "the view has no depth layer in RP_DEPTH_METRES";
  if (!bad && !e.seg) bad = "the view has no segmentation layer";
  if (!bad && !xyz && !count) bad = "no output (xyz and count are both NULL)";
  if (!bad && point_rgb && !e.rgb) bad = "point_rgb is given but the view has no rgb layer";
  if (!bad && fin && (!f.depth || !f.seg)) bad = "a final_* output is given but the view has no final depth and segmentation layers";
  if (!bad && final_point_rgb && !f.rgb) bad = "final_point_rgb is given but the view has no final rgb layer";
  if (bad) { snprintf(h->err, 256, "rp_set_image_points: view %d: %s", view, bad); return RP_ERR_ARG; }
  if (c.pc_has[view]) HIPCHK(h, hipDeviceSynchronize());      /* replaced: as above */
  else c.pc_n++;
  c.pc_obs[view] = points_entry(e, spec, xyz, point_seg, point_rgb, count);
  c.pc_has[view] = 1;
  if (fin) {
    c.pc_fin[view] = points_entry(f, spec, final_xyz, final_point_seg, final_point_rgb, final_count);
    c.pc_has[view] |= 2;
  }
  return RP_OK;
}

/* test seam and benchmark control: on = 0 puts every record on every tile's shortlist (the default is on) */
int rp_debug_render_cull(rp_handle h, int32_t on) { if (!h) return RP_ERR_ARG; h->render_nocull = on ? 0 : 1; return RP_OK; }

int rp_ray_test(rp_handle h, const float* from, const float* to, int32_t k, float* hit_fraction, int32_t* collider, int32_t* link,
                float* hit_position, float* hit_normal, void* stream) {
  if (!h || !from || !to || k <= 0) { if (h) snprintf(h->err, 256, "rp_ray_test: bad argument"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs;
  int rc = rc_reserve(h, N);
  if (rc != RP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  poses_launch(h, 0, N, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s);      /* (no EE poses, no colour in a ray test's answer) */
  hipLaunchKernelGGL(k_ray_test, dim3(N), dim3(64), 0, s, h->dev_model, h->rc_tab, h->rc_cnt, N, k, from, to, hit_fraction, collider, link, hit_position, hit_normal);
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_get_collider_dims(rp_handle h, int32_t* n_col) {
  if (!h || !n_col) return RP_ERR_ARG;
  *n_col = h->host_model.n_col;
  return RP_OK;
}

/* Closest points between colliders of m rows - the live envs or rows of a caller's buffer: per chunk of rows (rp_render_states' chunks of pose-table slots)
 * k_collider_poses_rows without a sub-goal and k_closest_points on `stream`, every output moved to the chunk's first row on the host.  Only the pose table is written
 * (and grown, by rc_reserve, to the chunk size); `pairs` is read by the kernel alone. */
int rp_closest_points(rp_handle h, const rp_state_rows* src, int32_t m, const int32_t* pairs, int32_t k, int32_t n_groups, float max_distance, float* distance,
                      float* point_a, float* point_b, float* normal, int32_t* status, float* group_min, int32_t* group_pair, void* stream) {
  if (!h) return RP_ERR_ARG;
  const int N = h->cfg.num_envs;
  const bool stored = src && src->rows;
  const char* bad = nullptr;
  if (m < 1) bad = "m < 1";
  else if (k < 1 || k > RP_CP_MAX_PAIRS) bad = "k lies outside 1 .. 4096";
  else if (n_groups < 0 || n_groups > RP_CP_MAX_GROUPS) bad = "n_groups lies outside 0 .. 64";
  else if ((group_min || group_pair) && n_groups == 0) bad = "group_min / group_pair given with n_groups == 0";
  else if (!pairs) bad = "pairs is NULL";
  else if (!distance && !point_a && !point_b && !normal && !status && !group_min && !group_pair) bad = "no output (every output is NULL)";
  else if (max_distance != max_distance) bad = "max_distance is not a number";
  else if (stored && src->row_stride < RP_REC_FLOATS * sizeof(float)) bad = "row_stride < 512";
  else if (stored && src->row_stride % 4 != 0) bad = "row_stride is not a multiple of 4";
  else if (stored && src->n_rows < 1) bad = "n_rows < 1";
  else if (!(src && src->row_index) && m > (stored ? src->n_rows : N)) bad = stored ? "m exceeds n_rows and row_index is NULL" : "m exceeds the handle's envs and row_index is NULL (live rows)";
  if (bad) { snprintf(h->err, 256, "rp_closest_points: %s", bad); return RP_ERR_ARG; }
  const float* rows = stored ? (const float*)src->rows : h->state;
  const size_t row_floats = stored ? src->row_stride / sizeof(float) : (size_t)RP_REC_FLOATS;
  const int n_rows = stored ? src->n_rows : N;
  const int* row_index = src ? src->row_index : nullptr;
  long long cap = h->rs_chunk > 0 ? h->rs_chunk : (N > 4096 ? N : 4096);
  if (cap > m) cap = m;
  DevGuard guard(h->cfg.device);
  int rc = rc_reserve(h, (int)cap);
  if (rc != RP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int G = (group_min || group_pair) ? n_groups : 0;
  const size_t lds = (size_t)G * 64 * (sizeof(float) + sizeof(int));
  for (long long base = 0; base < m; base += cap) {
    const int num = (int)(m - base < cap ? m - base : cap);
    const int* idx = row_index ? row_index + base : nullptr;
    const size_t o = (size_t)base * k, og = (size_t)base * n_groups;
    hipLaunchKernelGGL(k_collider_poses_rows<false>, dim3(num), dim3(64), 0, s, h->dev_model, rows, row_floats, n_rows, idx, (int)base, num, h->rc_tab, h->rc_cnt,
                       (const float*)nullptr, (float*)nullptr, (const float*)nullptr, (const int*)nullptr, N);
    hipLaunchKernelGGL(k_closest_points, dim3(num), dim3(64), lds, s, h->dev_model, h->rc_tab, h->rc_cnt, num, idx, (int)base, n_rows, (const int*)pairs, (int)k, G,
                       max_distance, distance ? distance + o : nullptr, point_a ? point_a + 3 * o : nullptr, point_b ? point_b + 3 * o : nullptr,
                       normal ? normal + 3 * o : nullptr, status ? (int*)status + o : nullptr, group_min ? group_min + og : nullptr,
                       group_pair ? (int*)group_pair + og : nullptr);
  }
  HIPCHK(h, hipGetLastError());
  return RP_OK;
}

int rp_get_timers(rp_handle h, rp_timers* t) {
  if (!h || !t) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  rp_timers r = h->timers;
  r.steps_timed = 0; r.avg_step_ms = r.avg_action_ms = r.avg_prep_ms = r.avg_solve_ms = r.avg_obs_ms = 0.f;
  if (h->pool && h->pool_count > 0) {
    double step = 0, act = 0, prep = 0, solve = 0, obs = 0;
    for (int k = 0; k < h->pool_count; k++) {
      hipEvent_t* ev = h->pool + (size_t)k * EV_PER_STEP;
      HIPCHK(h, hipEventSynchronize(ev[1]));
      float ms;
      hipEventElapsedTime(&ms, ev[0], ev[1]); step += ms;
      hipEventElapsedTime(&ms, ev[2], ev[3]); act += ms;
      for (int sub = 0; sub < K_NSUB; sub++) {
        hipEventElapsedTime(&ms, ev[4 + 4 * sub], ev[5 + 4 * sub]); prep += ms;
        hipEventElapsedTime(&ms, ev[6 + 4 * sub], ev[7 + 4 * sub]); solve += ms;
      }
      hipEventElapsedTime(&ms, ev[4 + 4 * K_NSUB], ev[5 + 4 * K_NSUB]); obs += ms;
    }
    int c = h->pool_count;
    r.steps_timed = (uint32_t)c;
    r.avg_step_ms = (float)(step / c); r.avg_action_ms = (float)(act / c); r.avg_prep_ms = (float)(prep / (c * K_NSUB));
    r.avg_solve_ms = (float)(solve / (c * K_NSUB)); r.avg_obs_ms = (float)(obs / c);
    r.last_step_ms = r.avg_step_ms;
  }
  *t = r;
  return RP_OK;
}
int rp_enable_timers(rp_handle h, int32_t on) {
  if (!h || on < 0) return RP_ERR_ARG;
  if (on > 0 && h->fused == 2) { snprintf(h->err, 256, "rp_enable_timers: the k_chain pipeline (rp_set_fused(h, 2)) is one launch for twelve substeps - no per-launch timers"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  if (h->pool) { for (int i = 0; i < h->pool_steps * EV_PER_STEP; i++) hipEventDestroy(h->pool[i]); free(h->pool); h->pool = nullptr; }
  h->timers_on = on; h->pool_steps = on; h->pool_next = 0; h->pool_count = 0;
  if (on > 0) {
    h->pool = (hipEvent_t*)calloc((size_t)on * EV_PER_STEP, sizeof(hipEvent_t));
    for (int i = 0; i < on * EV_PER_STEP; i++) HIPCHK(h, hipEventCreate(&h->pool[i]));
  }
  return RP_OK;
}
const char* rp_last_error(rp_handle h) { return h ? h->err : g_err; }

int rp_debug_reset_rounds(rp_handle h) { return h ? h->reset_rounds : RP_ERR_ARG; }

/* test hook: k_autoreset's launch shape as rp_create fixed it - grid (blocks) and envs per block (RP_AUTORESET_BLOCKS / RP_AUTORESET_EPB) */
int rp_debug_autoreset_shape(rp_handle h, int32_t* grid, int32_t* epb) {
  if (!h || !grid || !epb) return RP_ERR_ARG;
  *grid = h->ar_grid; *epb = h->ar_epb;
  return RP_OK;
}

/* test hooks (include/rp_playroom_debug.h): one substep on every env, intermediates of env `env` into host buf[4096] */
int rp_debug_substep(rp_handle h, int32_t env, float* host_buf) {
  if (!h || !host_buf) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  int N = h->cfg.num_envs;
  HIPCHK(h, hipMemset(h->dbg, 0, 4096 * sizeof(float)));
  hipLaunchKernelGGL(k_debug_substep, dim3(N), dim3(64), 0, 0, h->dev_model, h->state, h->dbg, N, env);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(host_buf, h->dbg, 4096 * sizeof(float), hipMemcpyDeviceToHost));
  return RP_OK;
}

/* test hook: the action stage alone (k_action's body in k_action's launch shape) on the current state, on the NULL stream.  The envs are cut into blocks by the LATEST step's
 * member table and group bounds as they stand (the next step would re-rank first); before the first step of a pipeline, in identity order and rp_set_groups' groups.
 * raw_dev [N][8]: the solution before the clamps to the joint limits and to q +- inc (7), then 1 * capped + 2 * marginal + 4 * place.  Motor targets and status word go
 * into the state as in a step; nothing else is written.  Synchronises the stream. */
int rp_debug_action(rp_handle h, const float* action_dev, float* raw_dev) {
  if (!h || !action_dev || !raw_dev) { if (h) snprintf(h->err, 256, "rp_debug_action: action_dev or raw_dev is NULL"); return RP_ERR_ARG; }
  DevGuard guard(h->cfg.device);
  const int N = h->cfg.num_envs;
  int G = h->sort_G;
  GroupBounds gb = h->gb;
  const int* member = h->member[h->member_cur];
  if (G == 0) {
    G = h->fused == 0 ? h->groups : 1;
    if (G > (N + 63) / 64) G = (N + 63) / 64;
    gb = split_groups(h, G, N);
    member = nullptr;
  }
  for (int g = 0; g < G; g++) {
    const int e0 = gb.b[g], e1 = gb.b[g + 1];
    if (e1 > e0) hipLaunchKernelGGL(k_debug_action, dim3((e1 - e0 + 3) / 4), dim3(64), 0, 0, h->dev_model, h->state, action_dev, e0, e1, member, raw_dev);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(0));
  return RP_OK;
}

/* test hook: the joints of the ghost arm(s) of the latest rp_render_ex with a ghost_arm, [num_envs of that call][8], into host_buf */
int rp_debug_ghost_joints(rp_handle h, float* host_buf, int32_t num_envs) {
  if (!h || !host_buf || num_envs < 1 || num_envs > h->rc_cap || !h->rc_ee) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpy(host_buf, h->rc_ee + (size_t)12 * h->rc_last_num, (size_t)num_envs * 8 * sizeof(float), hipMemcpyDeviceToHost));
  return RP_OK;
}

/* test hook: per-env (nsmall, ncon) of the most recent k_prep2 into host_buf[2*N] */
int rp_debug_row_counts(rp_handle h, int32_t* host_buf) {
  if (!h || !host_buf) return RP_ERR_ARG;
  DevGuard guard(h->cfg.device);
  HIPCHK(h, hipDeviceSynchronize());
  int N = h->cfg.num_envs;
  for (int e = 0; e < N; e++) {   /* header: maskL, maskU, nj, ncon, nA, nB, gear, nC -> (unit rows, ncon + 1000 * (arm contact) + 1e5 * spanning contacts) */
    int32_t hdr[8];
    HIPCHK(h, hipMemcpy(hdr, h->ws + (size_t)e * W3_FLOATS, 8 * sizeof(int32_t), hipMemcpyDeviceToHost));
    host_buf[2 * e] = 12 + __builtin_popcount((unsigned)hdr[0]) + __builtin_popcount((unsigned)hdr[1]) + hdr[2];
    host_buf[2 * e + 1] = hdr[3] + 1000 * ((hdr[4] + hdr[7]) > 0) + 100000 * hdr[7];
  }
  return RP_OK;
}

#ifdef RP_PROLOGUE_CLOCKS
int rp_debug_prologue_clocks(rp_handle h, uint64_t* host_buf, int32_t nwaves) {
  if (!h || !host_buf || nwaves > 4096) return RP_ERR_ARG;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_pclk), (size_t)nwaves * 8 * sizeof(uint64_t)));
  return RP_OK;
}
#endif
#ifdef RP_CHAIN_CLOCKS
int rp_debug_chain_clocks(rp_handle h, int64_t* host_buf, int32_t nblocks) {
  if (!h || !host_buf || nblocks > 4096) return RP_ERR_ARG;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_chain_clk), (size_t)nblocks * 4 * sizeof(int64_t)));
  return RP_OK;
}
#endif
#ifdef RP_CLOCKS
#if RP_CLOCKS == 2
#define RP_CLK_STRIDE 32
#else
#define RP_CLK_STRIDE 8
#endif
int rp_debug_clocks(rp_handle h, uint64_t* host_buf, int32_t nblocks) {
  if (!h || !host_buf || nblocks > 4096) return RP_ERR_ARG;
  HIPCHK(h, hipDeviceSynchronize());
  HIPCHK(h, hipMemcpyFromSymbol(host_buf, HIP_SYMBOL(g_clk), (size_t)nblocks * RP_CLK_STRIDE * sizeof(uint64_t)));
  return RP_OK;
}
#endif

}  /* extern "C" */
