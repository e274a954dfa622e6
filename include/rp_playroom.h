/* rp_playroom.h — C ABI of the MI355X-native batched playroom simulator (librp_playroom_hip.so).
 *
 * This is the drop-in boundary of SURVEY.md §8b.  The reference has no FFI of its own: its hot path calls the
 * PyBullet client (third-party, CPU) from Python.  Each entry point below REPLACES a group of those calls for N
 * environments at once; the reference interface it stands in for is cited per function
 * (ENV = roboticsPlayroomPybullet/envs/environments.py, IKS = inverseKinematics.py, RWD = playRewardFunc.py).
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions; every function returns 0 on success or a negative rp_status.
 *   - all array arguments are DEVICE pointers to caller-owned, contiguous, row-major [N, dim] buffers
 *     (float32 unless noted), valid until `stream` reaches the call; the library owns only its internal state.
 *   - a handle is bound to one device, is not thread-safe, and enqueues on the caller's stream
 *     (pass torch.cuda.current_stream().cuda_stream); `stream` is a hipStream_t passed as void*.
 *   - no host<->device copies and no synchronisation inside rp_step / rp_step_autoreset / rp_reset_to / rp_compute_reward; rp_reset reads one
 *     4-byte counter back per round of settle substeps (see rp_reset).  (Debug path only: with rp_set_fused(h, 1) AND timers
 *     enabled, rp_step waits for its own kernel to read the timer - rp_playroom_debug.h.)
 *   - every entry point makes the handle's device current for the duration of the call and restores the caller's device,
 *     so handles on different devices (or several on one device, each driven on its own stream) can live in one process.
 *   - per-env numerical blow-ups are not errors: they set status[env] != 0 in rp_out.
 */
#ifndef RP_PLAYROOM_H
#define RP_PLAYROOM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rp_sim* rp_handle;

enum rp_status { RP_OK = 0, RP_ERR_ARG = -1, RP_ERR_HIP = -2, RP_ERR_UNSUPPORTED = -3, RP_ERR_STATE_SIZE = -4,
                 RP_ERR_INCOMPLETE = -5 /* rp_reset ran out of rounds with envs still pending (their status[] is set to 4) */ };

/* registered ids in scope (roboticsPlayroomPybullet/__init__.py:92,66,24) and, from SURVEY.md 8f rank 1, the rest of
 * the UR5 one-object play family (__init__.py:72,77,82,87,97; envList.py:101-140): same scene and arm as
 * UR5PlayAbsRPY1Obj-v0, other action types (environments.py:915-981) */
enum rp_env_kind {
  RP_ENV_UR5_PLAY_ABS_RPY_1OBJ = 0, RP_ENV_UR5_REACH = 1, RP_ENV_PANDA_PICK = 2,
  RP_ENV_UR5_PLAY_1OBJ = 3,            /* absolute_quat   [x y z qx qy qz qw grip]  */
  RP_ENV_UR5_PLAY_REL_1OBJ = 4,        /* relative_quat   (added to the measured EE pose, componentwise) */
  RP_ENV_UR5_PLAY_REL_JOINTS_1OBJ = 5, /* relative_joints [dq0..dq5 grip], no IK */
  RP_ENV_UR5_PLAY_ABS_JOINTS_1OBJ = 6, /* absolute_joints [q0..q5 grip], no IK */
  RP_ENV_UR5_PLAY_REL_RPY_1OBJ = 7,    /* relative_rpy    [dx dy dz droll dpitch dyaw grip] */
  RP_ENV_PANDA_PUSH = 8,               /* pandaPush-v0 (__init__.py:19, envList.py:12-16): pandaPick's arm and scene, other ranges */
  /* the Panda in the other two scenes */
  RP_ENV_PANDA_REACH = 9,              /* pandaReach-v0 (__init__.py:4, envList.py:8-10): Panda + default_scene, no object */
  RP_ENV_PANDA_REACH_2D = 10,          /* pandaReach2D-v0 (__init__.py:9, envList.py:24-26): same, goals just above the plane */
  /* the Panda one-object play family (__init__.py:33-64, envList.py:43-88): Panda + complex_scene, one id per action type;
   * joint-space actions carry 7 joints: [q0..q6 grip] */
  RP_ENV_PANDA_PLAY_1OBJ = 11,            /* absolute_quat   */
  RP_ENV_PANDA_PLAY_REL_1OBJ = 12,        /* relative_quat   */
  RP_ENV_PANDA_PLAY_REL_JOINTS_1OBJ = 13, /* relative_joints */
  RP_ENV_PANDA_PLAY_ABS_JOINTS_1OBJ = 14, /* absolute_joints */
  RP_ENV_PANDA_PLAY_ABS_RPY_1OBJ = 15,    /* absolute_rpy    */
  RP_ENV_PANDA_PLAY_REL_RPY_1OBJ = 16,    /* relative_rpy    */
  /* the two-object play ids (__init__.py:29, 41; envList.py:28-41): Panda + complex_scene with two blocks.  Served by the
   * RP_WIDE build of this library (librp_playroom_hip_wide.so: three free bodies in the state record, observations 26 / 18 wide,
   * the drawer in the arm's half of the solver's lane layout); librp_playroom_hip.so answers RP_ERR_UNSUPPORTED for them, and
   * the wide build for every other id. */
  RP_ENV_PANDA_PLAY = 17,                 /* pandaPlay-v0: absolute_quat */
  RP_ENV_PANDA_PLAY_JOINTS = 18,          /* pandaPlayJoints-v0: relative_joints */
  RP_ENV_COUNT = 19
};

/* perform_action's dispatch (ENV:915-934); values of rp_config.action_type */
enum rp_action_type { RP_ACTION_ABSOLUTE_RPY = 0, RP_ACTION_RELATIVE_RPY = 1, RP_ACTION_ABSOLUTE_QUAT = 2, RP_ACTION_RELATIVE_QUAT = 3,
                      RP_ACTION_ABSOLUTE_JOINTS = 4, RP_ACTION_RELATIVE_JOINTS = 5 };

/* rp_config.flags: which of the optional fields are valid.  0 = the id exactly as envList.py registers it. */
enum rp_config_flags {
  RP_CFG_GOAL_RANGE = 1,    /* goal_range_low / goal_range_high    (ENV:495-498 goal draw, ENV:577-581 arm reset target) */
  RP_CFG_OBJ_RANGE = 2,     /* obj_lower_bound / obj_upper_bound   (ENV:527-533 object spawn) */
  RP_CFG_ENV_RANGE = 4,     /* env_range_high                      (ENV:537-540 out-of-bounds re-sample after settling) */
  RP_CFG_REW_THRESH = 8,    /* sparse_rew_thresh                   (ENV:297; ids that are not play ids) */
  RP_CFG_DENSE_REWARD = 16, /* sparse=False: compute_reward = -||ag - dg|| over the whole goal vector (ENV:169-170, 273-275) */
  RP_CFG_ACTION_TYPE = 32,  /* action_type                         (ENV:88-113, 915-981) */
  RP_CFG_CONTACT_MARGIN = 64, /* contact_margin, see below */
  RP_CFG_STATELESS_CONTACTS = 128 /* (no field) rebuild the contact points every substep instead of keeping them across substeps.  Default (flag clear): a
                                   * per-env contact cache (2.1 KB beside the state record) with btPersistentManifold's life cycle - one manifold per object pair
                                   * in creation order, <= 4 points in the two bodies' frames, refreshed every substep, dropped beyond the pair's breaking
                                   * threshold; a box pair makes new points only while the boxes overlap.  The cache is part of the state (rp_get_state /
                                   * rp_set_state rows carry it behind the record).  With the flag: round 3's first model - points
                                   * exist out to the pair's margin, nothing is remembered (13 % faster, further from Bullet: DESIGN.md section 2) */
  ,
  RP_CFG_HULL_GJK = 256,          /* (no field; the DEFAULT since 0.3, accepted for callers written against 0.2) an arm link whose deepest hull vertex lies BESIDE the
                                   * box face it approaches (box edges and corners) gets its contact from GJK's distance phase on hull and box (oracle
                                   * RPO_RULE_GJK): the reference loads mesh colliders (environments.py:397, 409-411) and Bullet runs GJK on their hulls */
  RP_CFG_SPECULATIVE_LIMITS = 1024, /* (no field) round 2's joint-limit rows: a row exists from 0.1 rad (m) BEFORE the limit on and lets the joint close the gap within the
                                   * substep (a contact-like speculative row, erp of the contacts).  Default (flag clear): Bullet's rule as recalled - a row only
                                   * while the limit is violated, erp 0.2 (btMultiBodyJointLimitConstraint::createConstraintRows) - under which a gripper joint whose
                                   * position motor is commanded past its limit (every "open" action, environments.py:1037-1073) chatters at the limit: 1.1 mm for a
                                   * Robotiq pad = 0.026 in obs_quat's gripper entry.  The flag trades that sawtooth for 1e-2 of free-motion divergence from the
                                   * reference step: an A / B switch for learners that see the gripper observation */
  RP_CFG_OBB_EDGES = 512,         /* (no field) round 3's contacts for that case: the link's OBB against the box (SAT + face clipping) instead of GJK on the hull -
                                   * a few per cent faster, further from Bullet (the headline id's block position: 8 cm instead of 2 mm median divergence from the
                                   * reference step over 200 steps) */
  RP_CFG_HULL_EPA = 2048,         /* (no field) where GJK finds the CORES of a link's hull and a box overlapping, depth, normal and witness come from the expanding polytope
                                   * on the two cores (Bullet's btGjkEpaSolver2; oracle RPO_RULE_EPA) instead of the OBB path.  The DEFAULT of the Panda ids (pandaPick: the
                                   * worst arm divergence from the reference step over 200 steps 1.2e-3 -> 5.6e-5 rad), not of the UR5 ids (nothing moves in their table rows;
                                   * 4 % of the headline, 19 % under the literal random-action rollout): this flag turns it on for those too ... */
  RP_CFG_NO_HULL_EPA = 4096       /* ... and this one off for the Panda ids.  Both set: RP_ERR_ARG.  Ignored under RP_CFG_OBB_EDGES (no GJK, no polytope). */
};

typedef struct rp_config {
  int32_t env_kind;      /* rp_env_kind */
  int32_t num_envs;      /* N, 1 .. 4194304 */
  int32_t device;        /* HIP device ordinal */
  int32_t env_offset;    /* global index of env 0 of this handle (multi-GPU shards: rank * N); keys the per-env RNG */
  uint64_t seed;         /* counter RNG: u = f(seed, env_offset + env, draw#) — shard-invariant */
  /* the kwargs an env class of envList.py hands to playEnv.__init__ (ENV:64-67) that reach the simulation; each is read only
   * when its rp_config_flags bit is set.  Kwargs that change the layout of the observation (num_objects, use_orientation,
   * return_velocity, play, arm_type) belong to the id and cannot be overridden. */
  uint32_t flags;
  int32_t action_type;   /* rp_action_type */
  float goal_range_low[3], goal_range_high[3];
  float obj_lower_bound[3], obj_upper_bound[3];
  float env_range_high[3];
  float sparse_rew_thresh;
  /* one distance, in metres, out to which the narrowphase creates contact points for every collider pair (0 .. 0.05).
   * Default (flag clear): per pair, Bullet's contact breaking threshold - gContactBreakingThreshold (0.02) x the smaller of
   * the two collision objects' angular-motion discs (btCollisionDispatcher's CD_USE_RELATIVE_CONTACT_BREAKING_THRESHOLD
   * default): 1.2 mm for the block, 0.4 - 6 mm for the arm links, 9 mm for the table.  Bullet keeps the points of its
   * persistent manifolds out to that distance, and so does this library's contact cache (default).  Setting this field is a
   * study of the STATELESS contacts (it implies RP_CFG_STATELESS_CONTACTS): points are rebuilt every substep and the margin
   * is the distance within which a point exists.  See DESIGN.md H7. */
  float contact_margin;
} rp_config;

/* per-kind output widths */
typedef struct rp_dims {
  int32_t obs_quat, achieved_goal, desired_goal, controllable_achieved_goal, full_positional_state, joints, velocity,
      observation, target_poses, action;
} rp_dims;

/* outputs of one step / reset: the reference's obs dict (ENV:849-861) + reward/info (ENV:211-214). NULL = skip. */
typedef struct rp_out {
  float* obs_quat;                   /* [N, dims.obs_quat] */
  float* achieved_goal;              /* [N, dims.achieved_goal] */
  float* desired_goal;               /* [N, dims.desired_goal] */
  float* controllable_achieved_goal; /* [N, 4] */
  float* full_positional_state;      /* [N, dims.full_positional_state] */
  float* joints;                     /* [N, 8] */
  float* velocity;                   /* [N, 6] */
  float* observation;                /* [N, dims.observation] */
  int32_t* gripper_proprioception;   /* [N] */
  float* reward;                     /* [N] */
  int32_t* is_success;               /* [N] */
  float* target_poses;               /* [N, dims.target_poses]; written by rp_step only */
  int32_t* status;                   /* [N] bit flags, 0 = ok: 1 non-finite state, 2 an object fell through the scene's ground plate
                                      * (tunnelled: it is below the lowest static collider), 4 rp_reset left this env unfinished,
                                      * 8 (informational, not a fault) the IK of the latest rp_step ran out of its iterations for this env
                                      * (inverseKinematics.py:44-50: 4 x 20; Panda: 200) - its joint targets then hang on the measured joints,
                                      * 16 (informational) one of that IK's stopping tests was decided within 0.5 % of the residual threshold: another
                                      * evaluation order of the same arithmetic may have stopped an iteration apart (~5e-5 rad in the joint targets) */
  float* pack;                       /* [N, dims.obs_quat + dims.achieved_goal + 2]: obs_quat | achieved_goal | reward | is_success
                                      * in one row, the message of the per-step multi-GPU observation gather,
                                      * written by the same kernel so the gather needs no packing pass */
} rp_out;

typedef struct rp_timers {
  float last_step_ms;    /* device time of the most recent rp_step (hipEvent pair on the call's stream) */
  float last_reset_ms;
  uint64_t steps;        /* rp_step calls so far */
  /* averages over the steps recorded since rp_enable_timers (per-launch hipEvent pairs on the call's stream;
   * nothing synchronises inside rp_step, rp_get_timers does) */
  uint32_t steps_timed;
  float avg_step_ms;     /* k_action .. k_calc_state, one rp_step */
  float avg_action_ms;   /* k_action, one launch */
  float avg_prep_ms;     /* k_prep, one launch (12 per step) */
  float avg_solve_ms;    /* k_solve, one launch (12 per step) */
  float avg_obs_ms;      /* k_calc_state, one launch */
} rp_timers;

/* gym.make(id) + playEnv.__init__ + activate_physics_client (ENV:64-170, 218-249): builds N identical worlds. */
int rp_create(const rp_config* cfg, rp_handle* out);
int rp_destroy(rp_handle h);
int rp_get_dims(rp_handle h, rp_dims* dims);

/* playEnv.reset(o=None) (ENV:173-187) for every env whose mask byte is non-zero (mask NULL = all):
 * resample block / arm / goal, 100 settle substeps, repeat while the goal is already satisfied.  The settle substeps run
 * through the step pipeline's kernels over the envs that still need them, in rounds; the host waits on `stream` once per round
 * (1-3 rounds for a few envs, more for the unluckiest env of a large batch), so the call returns when the reset is done.
 * Uses the handle's row workspace: do not overlap with rp_step on another stream. */
int rp_reset(rp_handle h, const uint8_t* mask, const rp_out* out, void* stream);

/* playEnv.reset(o) (ENV:173-187 with ENV:542-556, 575-590): objects and arm placed from an observation vector o [N, n_o]
 * instead of being sampled - object pose from o[11:18] (use_orientation ids) or o[7:10], arm IK target o[0:3] with
 * orientation o[3:7]; no settling; the goal is still drawn.  SURVEY.md 8f rank 2 (state restore). */
int rp_reset_to(rp_handle h, const float* o, int32_t n_o, const uint8_t* mask, const rp_out* out, void* stream);

/* playEnv.reset_goal_pos(goal) (ENV:190-191, 492-516). goal [N, dims.desired_goal] or NULL (random goal).
 * Play envs then overwrite the goal with a random perturbation of the achieved goal, as the reference does. */
int rp_reset_goal(rp_handle h, const float* goal, const uint8_t* mask, void* stream);

/* playEnv.step(action) (ENV:206-214): clip -> absolute_rpy IK (IKS:44-50 / ENV:995-997) -> motor targets
 * (ENV:1010-1073) -> 12 x stepSimulation at 300 Hz (ENV:485-490) -> calc_state (ENV:799-864) -> reward.
 * action [N, dims.action]: x y z roll pitch yaw gripper for the absolute_rpy ids; see rp_env_kind for the others. */
int rp_step(rp_handle h, const float* action, const rp_out* out, void* stream);

/* instance.calc_state() without stepping (ENV:799-864); updates the quaternion sign memory like the reference. */
int rp_calc_state(rp_handle h, const rp_out* out, void* stream);

/* playEnv.compute_reward(achieved_goal, desired_goal) (ENV:278-304, RWD:66-77) for M rows. */
int rp_compute_reward(rp_handle h, const float* achieved_goal, const float* desired_goal, float* reward, int32_t m, void* stream);
/* playEnv.compute_reward_sparse (environments.py:278-304): the sparse formula whatever `sparse` the env was built with (the reference rebinds only
 * compute_reward when sparse=False, environments.py:169-170; compute_reward_sparse stays callable) */
int rp_compute_reward_sparse(rp_handle h, const float* achieved_goal, const float* desired_goal, float* reward, int32_t m, void* stream);

/* full simulator state (positions, velocities, motor targets, goal, quaternion memory, RNG counters - the first 512 bytes of a row: the state record -
 * and, unless RP_CFG_STATELESS_CONTACTS, the env's contact cache behind it): the explicit save/restore the reference lacks.
 * src_env_count == 1 broadcasts one env to all N.  A row whose cache part is all zeros is a state without contact history. */
size_t rp_state_bytes(rp_handle h);           /* bytes per env (a row of the buffers below) */
int rp_get_state(rp_handle h, void* dst, void* stream);
int rp_set_state(rp_handle h, const void* src, int32_t src_env_count, void* stream);

/* ---- images and ray queries ----------------------------------------------------------------------
 * The reference renders obs['img'] with PyBullet's OpenGL rasteriser and asks Bullet for one ray per step; this library casts rays
 * against the boxes and spheres of its contact model, coloured like the reference's visual shapes (flat shading, no textures). */
typedef struct rp_camera {
  float eye[3], target[3], up[3];   /* computeViewMatrix(eye, target, up) */
  float fov_deg, aspect;            /* computeProjectionMatrixFOV(fov, aspect, near, far); near / far only clip: rays run 0 .. 10 m */
  int32_t mode;                     /* 0 = this camera; 1 = gripper camera (ENV:33-49): eye at the EE link; with (roll, pitch, yaw) the link's Euler angles it looks along Rz(yaw) Ry(pitch) z, up = Rz(yaw) Ry(pitch) (-cos roll, -sin roll, 0) */
} rp_camera;
/* the reference's fixed camera (ENV:21-30): computeViewMatrixFromYawPitchRoll(target [0, 0.25, 0], distance 1.3, yaw -30, pitch -30, roll 0,
 * upAxisIndex 2), computeProjectionMatrixFOV(fov 50, aspect 1, near 0.01, far 10) */
int rp_default_camera(rp_camera* cam);
/* p.computeViewMatrixFromYawPitchRoll's camera placement (degrees, upAxisIndex 2) */
int rp_camera_from_yaw_pitch_roll(const float target[3], float distance, float yaw_deg, float pitch_deg, float roll_deg, rp_camera* cam);
/* instance.calc_state()'s img (ENV:841-845: getCameraImage(width, height, view, projection)[2][:, :, :3]) for envs [first_env, first_env +
 * num_envs): rgb [num_envs, height, width, 3] uint8, row 0 = top.  cam NULL = rp_default_camera.  sub_goal (may be NULL):
 * [num_envs, dims.achieved_goal] - visualise_sub_goal(sub_goal, 'achieved_goal') (ENV:606-690): the objects and, for the play ids,
 * drawer / door / button / dial drawn a second time, half transparent, at the poses the vectors name. */
int rp_render(rp_handle h, const rp_camera* cam, int32_t width, int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb,
              const float* sub_goal, void* stream);
/* ... with the ghost ARM of visualise_sub_goal(sub_goal, 'controllable_achieved_goal' / 'full_positional_state') (ENV:623-637, 671-674): ghost_arm (may be NULL)
 * [num_envs, 8] = EE position 3, orientation quaternion 4 (xyzw), gripper 1 (unused, as in the reference's reset_arm) - a second arm, half transparent, at the joints one
 * default IK call from the rest pose finds for that pose (ENV:575-590).  Panda models only: RP_ERR_UNSUPPORTED for a UR5 (the reference raises NotImplementedError).
 * RP_ERR_ARG (rp_render too): rgb NULL, width or height outside 1 .. 4096, an env range outside the handle's, a camera with a mode other than 0 or 1, fov_deg outside
 * (0, 180) or aspect <= 0 - and, since both calls draw through rp_render_layers' kernel, num_envs * ceil(width / 16) * ceil(height / 16) > 2^31 - 1 tiles (an rgb buffer
 * of more than a terabyte; the grid of the kernel they had was an unsigned number of 256-pixel runs and was not checked). */
int rp_render_ex(rp_handle h, const rp_camera* cam, int32_t width, int32_t height, int32_t first_env, int32_t num_envs, uint8_t* rgb,
                 const float* sub_goal, const float* ghost_arm, void* stream);
/* all three layers of getCameraImage (ENV:841-845 takes [2], the colour) for envs [first_env, first_env + num_envs), row 0 = top; each output may be NULL, not all three:
 *   rgb [num_envs, height, width, 3] uint8: byte for byte what rp_render_ex writes for the same arguments - by construction: rp_render and rp_render_ex are this call
 *     with the colour layer alone (ghosts blended at 0.5, rays 0 .. 10 m).
 *   depth [num_envs, height, width] float: the nearest NON-ghost hit of the pixel's ray as eye-space z = t (d . forward), d the normalised ray direction, t the hit
 *     parameter (on a sphere evaluated through the point of closest approach, which does not cancel at a grazing ray as rp_ray_test's float32 quadratic does: the two
 *     differ there by up to some 1e-4 m, elsewhere by rounding).  RP_DEPTH_BUFFER: PyBullet's depthBuffer value far (z - near) / (z (far - near)) clamped to [0, 1]; exactly 1.0 on a miss.  RP_DEPTH_METRES: z itself;
 *     exactly far_plane on a miss.  near_plane / far_plane only shape this value; they do not clip rays (as for rp_camera above).
 *   segmentation [num_envs, height, width] int32: -1 on a miss, else collider | ((link + 1) << 24) with the collider and link rp_ray_test reports for that ray
 *     (PyBullet's packing, the collider index standing where the body's unique id stands).
 * Ghosts (sub_goal, ghost_arm: as for rp_render_ex) are see-through markers: they tint rgb and never appear in depth or segmentation, as rp_ray_test ignores them.
 * Cameras: cam as for rp_render (NULL = rp_default_camera; the gripper camera, mode 1, is per env already), OR cam_rows, a DEVICE array [num_envs, 11], row i for env
 * first_env + i: eye[3] target[3] up[3] fov_deg aspect, from which the kernel builds the basis rp_render builds on the host from an rp_camera (same operations, in
 * double, zero-length vectors included).  Never both.  The library does not range-check device values (fov in (0, 180), aspect > 0 are the caller's to keep).
 * RP_ERR_ARG: all three outputs NULL, both cam and cam_rows, near_plane <= 0, far_plane <= near_plane, an unknown depth mode, rp_render_ex's size, range and camera errors.
 * RP_ERR_UNSUPPORTED: a ghost arm on a UR5.  Enqueued on `stream`: no host wait, no host read of device values. */
enum rp_depth_mode { RP_DEPTH_BUFFER = 0, RP_DEPTH_METRES = 1 };
int rp_render_layers(rp_handle h, const rp_camera* cam, const float* cam_rows /* device [num_envs, 11] or NULL */,
                     float near_plane, float far_plane, int32_t depth_mode,
                     int32_t width, int32_t height, int32_t first_env, int32_t num_envs,
                     uint8_t* rgb /* [num_envs, height, width, 3] or NULL */,
                     float* depth /* [num_envs, height, width] or NULL */,
                     int32_t* segmentation /* [num_envs, height, width] or NULL */,
                     const float* sub_goal, const float* ghost_arm, void* stream);
/* ---- camera images written by the calls that write observations ------------------------------------------------------------------------
 * While set, every call that writes observation rows also draws the images of the same envs, on the call's stream, after the observations and from the state those
 * observations describe:
 *   rp_step, rp_calc_state          all envs
 *   rp_reset, rp_reset_to           the envs of the mask (NULL = all); the rows of unmasked envs are not touched.  rp_reset on RP_ERR_INCOMPLETE too: the image shows
 *                                   whatever state the row has
 *   rp_step_autoreset               in the order step, k_autoreset_mark, TERMINAL PASS, the reset kernels, OBSERVATION PASS.  The terminal pass draws, for every env
 *                                   with done != 0, the layers whose final_* pointer is non-NULL into that env's row of final_*, from the state the step left, before
 *                                   the reset; rows of envs that did not end are not written.  The observation pass covers all envs: an ended env gets the first frame
 *                                   of its new episode, as out's observation arrays do.  The step inside the call does not draw on its own: an env is drawn once for
 *                                   the terminal pass, only if it ended, and once for the observation pass.  All three final_* NULL: no terminal pass.
 * A row of rgb / depth / segmentation is byte for byte what rp_render_layers(h, cam, cam_rows, near_plane, far_plane, depth_mode, width, height, e, 1, ...) would write
 * for that env at that moment, without ghosts (sub_goal, ghost_arm = NULL) and with the handle's visuals table (rp_set_visuals); row e of cam_rows belongs to env e.
 * cam is copied at the call; NULL with no cam_rows = rp_default_camera; mode 1 is the gripper camera, which is per env already.  cam_rows (device [N, 11], rp_render_layers'
 * layout) is caller-owned, stays referenced until the next rp_set_image_obs and is read on the device at every draw: a caller may rewrite its values between calls (a new
 * camera for each new episode); the host never reads it.  The output buffers are caller-owned, like the arrays of rp_out: rgb [N, height, width, 3] uint8, depth
 * [N, height, width] float, segmentation [N, height, width] int32, each may be NULL, not all three; final_* have the same shapes and each may be NULL.
 * Cost: a stepping call makes two more launches per pass - no host wait, no host read of device values, no allocation; the envs of a pass are selected on the device
 * (done, mask).  rp_set_image_obs itself reserves the pose table for N envs, and may synchronise the device when it replaces or switches off a configuration that calls
 * in flight may still read, as rp_set_reset_table does.  width == 0 && height == 0 switches the feature off; the other arguments are then ignored, and the table's memory
 * stays until rp_destroy.  A handle that never calls this launches exactly what it launched before.
 * RP_ERR_ARG (the configuration in force stays): rgb, depth and segmentation all NULL while switching on; both cam and cam_rows; rp_render_layers' size, camera,
 * near / far and depth-mode errors; N * ceil(width / 16) * ceil(height / 16) > 2^31 - 1.
 * The configuration is not state: rp_get_state, rp_set_state and rp_copy_envs do not carry it.  The image passes share the handle's ONE collider-pose table with
 * rp_render, rp_render_ex, rp_render_layers and rp_ray_test: do not overlap one of those, or a second call that draws, with a call that draws on another stream. */
int rp_set_image_obs(rp_handle h, const rp_camera* cam, const float* cam_rows /* device [N, 11] or NULL */,
                     float near_plane, float far_plane, int32_t depth_mode, int32_t width, int32_t height,
                     uint8_t* rgb, float* depth, int32_t* segmentation,                      /* [N, h, w, 3] / [N, h, w] / [N, h, w], each may be NULL, not all */
                     uint8_t* final_rgb, float* final_depth, int32_t* final_segmentation);   /* same shapes, each may be NULL: the ended envs' rows under rp_step_autoreset */
/* ---- several camera views per env written by the same calls -----------------------------------------------------------------------------
 * rp_set_image_obs for up to RP_MAX_IMAGE_VIEWS views at once (a fixed camera and the gripper camera, say, at different sizes and with different layers): its
 * semantics view by view.  While set, rp_step and rp_calc_state draw every view of all envs, rp_reset and rp_reset_to every view of the mask's envs (on
 * RP_ERR_INCOMPLETE too), on the call's stream, after the observations; rp_step_autoreset makes its TERMINAL PASS after k_autoreset_mark - the envs with done != 0, and
 * only the views and layers whose final_* pointer is non-NULL - and its OBSERVATION PASS, all envs and every view, after the reset kernels.  Row e of every layer of view
 * k is byte for byte what rp_render_layers(h, that view's cam, cam_rows, near_plane, far_plane, depth_mode, width, height, e, 1, ...) would write for env e at that
 * moment, without ghosts and with the handle's visuals table; rows of unselected envs are not touched.
 * The handle has ONE image configuration: rp_set_image_views and rp_set_image_obs each replace it, the latest call wins.  n_views == 0 (views may be NULL) switches the
 * feature off, as rp_set_image_obs with width == 0 && height == 0 does.  The views array and each cam are copied at the call (cam NULL with no cam_rows =
 * rp_default_camera; mode 1 = the gripper camera); cam_rows and the output buffers stay the caller's and stay referenced, as rp_set_image_obs' do.  Replacing or
 * switching off a configuration in force synchronises the device first.  The configuration is not state: rp_get_state, rp_set_state and rp_copy_envs do not carry it;
 * rp_destroy frees nothing new.  The pose table is reserved for N envs here: no stepping call allocates, waits for the host or reads device values.
 * Cost: one view is rp_set_image_obs' configuration, with its two launches per pass.  Two or more views cost TWO launches per pass whatever their number: one
 * k_collider_poses over the N envs - the poses do not depend on the camera - and one k_render_views whose grid holds the tiles of all views of the pass.
 * RP_ERR_ARG (the configuration in force stays; the message names the view): n_views < 0 or > RP_MAX_IMAGE_VIEWS; views NULL with n_views > 0; for any view what
 * rp_set_image_obs refuses (no layer, both cam and cam_rows, the size, camera, near / far and depth-mode errors); N times the SUM of the views' tile counts
 * ceil(width / 16) * ceil(height / 16) > 2^31 - 1.  Shares the handle's one collider-pose table as rp_set_image_obs does: no overlap with a drawing call on another stream. */
#define RP_MAX_IMAGE_VIEWS 4
typedef struct rp_image_view {
  const rp_camera* cam;        /* copied at the call; NULL with no cam_rows = rp_default_camera; mode 1 = gripper camera */
  const float* cam_rows;       /* device [N, 11], caller-owned, read on the device at every draw; never both */
  float near_plane, far_plane;
  int32_t depth_mode;          /* rp_depth_mode */
  int32_t width, height;       /* 1 .. 4096 each; views may differ */
  uint8_t* rgb; float* depth; int32_t* segmentation;                    /* [N, h, w, 3] / [N, h, w] / [N, h, w]; each may be NULL, not all three */
  uint8_t* final_rgb; float* final_depth; int32_t* final_segmentation;  /* same shapes, each may be NULL */
} rp_image_view;
int rp_set_image_views(rp_handle h, const rp_image_view* views, int32_t n_views);
/* ---- per-env point clouds from the camera views ---------------------------------------------------------------------------------------------
 * A fixed number P = max_points of points per env, compacted on the device from a view's depth (RP_DEPTH_METRES: eye-space z) and segmentation layers by kernel
 * k_point_cloud, one block per (env, view), behind the draw that wrote the layers.  THE RULE, for one env and one view of width x height:
 *   pixels are taken in row-major order, i = y * width + x.  Pixel i is VALID iff segmentation[i] != -1 (a hit), bit (segmentation[i] & 0xFF) of drop is clear (its
 *   collider is not dropped) and (max_depth <= 0 || depth[i] <= max_depth).  n = the number of valid pixels, r(i) = the rank of a valid pixel among the valid ones.
 *   n <= P: slot r(i) takes pixel i; slots n .. P - 1 are PADDING: xyz = (0, 0, 0), point_seg = -1, point_rgb = (0, 0, 0).
 *   n >  P: slot j (0 <= j < P) takes the valid pixel of rank floor(j * n / P), in 64-bit integers: an even, deterministic stride through the hits in scan order
 *           (slot 0 is always the first hit).
 *   count = n, NOT capped at P: min(count, P) slots hold points, and count / P is the subsampling ratio.
 * Which pixel lands in which slot is integer logic: exact, no atomics, the same on every run.  Per point: point_seg = the pixel's packed segmentation value
 * (collider | (link + 1) << 24), point_rgb = the pixel's three bytes of the rgb layer, and xyz in float32, operation by operation without contraction, with the
 * renderer's own expressions nx = (2 (x + 0.5) / width - 1) tan_half_fov aspect, ny = (1 - 2 (y + 0.5) / height) tan_half_fov, z = depth[i]:
 *   RP_POINTS_CAMERA  (nx z, ny z, z) along the camera's (right, up, forward): the third component is the depth value bit for bit
 *   RP_POINTS_WORLD   eye + ((forward + right nx) + up ny) z, component by component, with the basis the renderer built for that env: the launch's camera, the env's
 *                     row of cam_rows (in double), or for the gripper camera (mode 1) the basis at the env's EE link - which the library does not expose otherwise.
 * rp_render_points draws and compacts in one call: k_collider_poses, k_render_layers (RP_DEPTH_METRES, near 0.01, far 10, no ghosts, the handle's visuals table) into
 * the CALLER'S layer buffers depth and segmentation [num_envs, height, width] - both required; rgb [num_envs, height, width, 3] may be NULL unless point_rgb is wanted -
 * and k_point_cloud into xyz [num_envs, P, 3] float, point_seg [num_envs, P] int32, point_rgb [num_envs, P, 3] uint8, count [num_envs] int32 (each may be NULL, not both
 * xyz and count).  cam / cam_rows, width, height, first_env, num_envs as for rp_render_layers.  Three launches on `stream`; no host wait, no host read of device values.
 * RP_ERR_ARG: spec NULL, max_points outside 1 .. 65536, an unknown frame, max_depth not a number; depth or segmentation NULL; xyz and count both NULL; point_rgb without
 * rgb; rp_render_layers' size, range and camera errors (both cam and cam_rows among them).  Shares the handle's one collider-pose table: do not overlap it with a
 * call that draws on another stream. */
enum rp_points_frame { RP_POINTS_WORLD = 0, RP_POINTS_CAMERA = 1 };
typedef struct rp_points_spec {
  int32_t max_points;   /* P, 1 .. 65536 */
  int32_t frame;        /* rp_points_frame */
  float max_depth;      /* metres of eye-space z; <= 0: no limit */
  uint64_t drop;        /* bit c: drop pixels whose hit collider is c (RP_MAX_COL = 64) */
} rp_points_spec;
int rp_render_points(rp_handle h, const rp_camera* cam, const float* cam_rows /* device [num_envs, 11] or NULL */,
                     int32_t width, int32_t height, int32_t first_env, int32_t num_envs, const rp_points_spec* spec,
                     uint8_t* rgb /* layer buffer [num_envs, height, width, 3] or NULL */,
                     float* depth /* layer buffer [num_envs, height, width], required */,
                     int32_t* segmentation /* layer buffer [num_envs, height, width], required */,
                     float* xyz /* [num_envs, P, 3] */, int32_t* point_seg /* [num_envs, P] */, uint8_t* point_rgb /* [num_envs, P, 3] */,
                     int32_t* count /* [num_envs] */, void* stream);
/* Attaches a cloud to view `view` of the image configuration IN FORCE (rp_set_image_obs' configuration is view 0; rp_set_image_views' views count from 0); spec NULL
 * detaches it.  While attached, every image pass - rp_step, rp_calc_state, the masked rp_reset / rp_reset_to, both passes of rp_step_autoreset - launches ONE more
 * k_point_cloud behind its draw: one launch for all attached views of the pass, with the pass's selection, from the layers the pass has just written.  The
 * observation pass writes xyz / point_seg / point_rgb / count [N, ...] (shapes as rp_render_points', each may be NULL, not both xyz and count); the terminal pass
 * writes final_* for the envs with done != 0 only, where any final_* is given (all four NULL: no terminal cloud).  Rows of unselected envs keep what they held.  A row
 * is what rp_render_points with the view's camera arguments would write for that env at that moment.  The buffers are caller-owned and stay referenced.
 * Cost: one launch per pass, no host wait, no host read of device values, no allocation.  Any later rp_set_image_obs or rp_set_image_views, switching off included,
 * drops ALL attachments, after the synchronisation those calls make; replacing or detaching an attachment synchronises the device first.  Not state: rp_get_state,
 * rp_set_state and rp_copy_envs do not carry it.  A handle that never calls this launches exactly what it launched before.
 * RP_ERR_ARG (the attachments stay as they were; the message names the cause): no configuration in force; view out of range; a bad spec (as rp_render_points); the
 * view's depth layer missing or not in RP_DEPTH_METRES; its segmentation layer missing; xyz and count both NULL; point_rgb given but the view has no rgb layer; a
 * final_* output given but the view lacks the final depth or segmentation layer, or final_point_rgb without the final rgb layer. */
int rp_set_image_points(rp_handle h, int32_t view, const rp_points_spec* spec,
                        float* xyz, int32_t* point_seg, uint8_t* point_rgb, int32_t* count,
                        float* final_xyz, int32_t* final_point_seg, uint8_t* final_point_rgb, int32_t* final_count);
/* bullet_client.rayTest(from, to) (ENV:738-741) for k rays per env: from / to [N, k, 3] world coordinates.  Outputs (each may be NULL):
 * hit_fraction [N, k] (1 on a miss), collider [N, k] (index into the model's collider table, -1 on a miss), link [N, k] (Bullet link
 * index of an arm collider, -1 otherwise), hit_position [N, k, 3], hit_normal [N, k, 3].  A ray that starts inside a shape does not hit it. */
int rp_ray_test(rp_handle h, const float* from, const float* to, int32_t k, float* hit_fraction, int32_t* collider, int32_t* link,
                float* hit_position, float* hit_normal, void* stream);
/* ---- camera images of stored state rows, and goal images -----------------------------------------------------------------------------------------
 * rp_render_layers for m images of states the handle need not be in: rows of a caller's device buffer in rp_get_state's layout (a replay buffer, a recorded
 * dataset), gathered by an index, each drawn with a named row of the handle's visuals table; and, with a goal in RP_GOAL_SOLID, the scene AT the goal.
 * IMAGE i (row i of rgb [m, height, width, 3] uint8, depth [m, height, width] float, segmentation [m, height, width] int32; each may be NULL, not all three) is byte
 * for byte what rp_render_layers(h, cam, cam_rows, near_plane, far_plane, depth_mode, width, height, e, 1, ...) writes for an env e whose state record is row
 * row_index[i] of src->rows and whose visuals row is that of env vis_env[i]: the same cam (NULL = rp_default_camera; mode 1, the gripper camera, sits at the EE
 * link OF THE ROW'S STATE) or row i of cam_rows (device [m, 11], rp_render_layers' layout; never both), the same near / far / depth mode / size; the toggles' red /
 * white follow the row's joint values, as on a live env.  Kernels k_collider_poses_rows and k_render_states: k_collider_poses' body and k_render_layers' tile.
 * THE HANDLE'S OWN STATE: the call never writes the handle's state rows, its contact cache, its counters or any table; a handle that is stepping is afterwards as
 * it was.  src->rows NULL draws the handle's live rows (row_stride and n_rows are then ignored: 512, N).
 * row_index[i] outside [0, n_rows): image i is NOT DRAWN - its rows of rgb / depth / segmentation keep what they held (rp_copy_envs' convention for a bad src);
 * the image's blocks leave before they read the row, ahead of their first barrier, and write nothing: a wrong index is an unwritten image, not a fault.
 * vis_env NULL, an entry outside [0, N), or a handle whose visuals table was never made (no rp_set_visuals / rp_get_visuals so far) give the DEFAULT row: the
 * baked colours and the default light and background, the arithmetic of a handle without a table.  The call does not make the table.
 * goal (device [m, dims.achieved_goal] or NULL), row i for image i.  RP_GOAL_GHOST: rp_render_layers' sub_goal, unchanged - half-transparent ghosts that tint rgb
 * only; there is no ghost arm in this call.  RP_GOAL_SOLID: the words a sub-goal overwrites for its ghost pass - the objects' positions, and their quaternions on
 * ids whose goal holds them; on play ids the drawer's y and the scene joints (door, button, dial) - are overwritten for the ONE and only pass: the image is that of
 * the row with those words replaced, opaque, present in depth and segmentation, the toggles coloured by the GOAL's joint values, no ghost records.  An id without
 * objects (UR5Reach-v0, the Panda reach ids) has nothing to move: the image is the plain one, as the ghost pass is a no-op there.
 * CHUNKS: 1 <= m <= 2^31 - 1, not bound to N.  The images are drawn in chunks of at most min(m, max(N, 4096)) pose-table slots, fewer where the chunk's tiles
 * chunk * ceil(width / 16) * ceil(height / 16) would exceed one launch; each chunk is two launches (poses, draw) on `stream`, the draw in k_render_layers'
 * tile-major block numbering.  No host wait, no host read of device values; the only allocation is the growth of the pose table to the chunk size at the first call
 * that needs it.  Shares the handle's ONE collider-pose table with every other call that draws and with rp_ray_test: do not overlap it with such a call on another
 * stream.
 * RP_ERR_ARG (nothing is launched; the message names the cause): src NULL; m < 1; rows non-NULL with row_stride < 512, a row_stride that is not a multiple of 4
 * or n_rows < 1; row_index NULL with m > n_rows (m > N for live rows); all three outputs NULL; both cam and cam_rows; an unknown goal_mode; rp_render_layers' size,
 * camera, near / far and depth-mode errors. */
enum rp_goal_mode { RP_GOAL_GHOST = 0, RP_GOAL_SOLID = 1 };
typedef struct rp_state_rows {
  const void*    rows;       /* device; rows in rp_get_state's layout.  Only the first 512 bytes of a row (the state record) are read.
                                NULL = the handle's own live state rows (then row_stride and n_rows are ignored: 512, N) */
  size_t         row_stride; /* bytes from one row to the next: >= 512 and a multiple of 4 */
  int32_t        n_rows;     /* rows in the buffer */
  const int32_t* row_index;  /* device [m] or NULL: image i draws row row_index[i]; NULL: row i (then m <= n_rows) */
  const int32_t* vis_env;    /* device [m] or NULL: image i is drawn with the visuals row of the handle's env vis_env[i] */
} rp_state_rows;
int rp_render_states(rp_handle h, const rp_state_rows* src, int32_t m,
                     const rp_camera* cam, const float* cam_rows /* device [m, 11] or NULL */,
                     float near_plane, float far_plane, int32_t depth_mode, int32_t width, int32_t height,
                     uint8_t* rgb, float* depth, int32_t* segmentation,       /* [m, h, w, 3] / [m, h, w] / [m, h, w]; each may be NULL, not all three */
                     const float* goal /* device [m, dims.achieved_goal] or NULL */, int32_t goal_mode, void* stream);

/* ---- closest points between colliders, live or from stored state rows ------------------------------------------------------------------------------
 * bullet_client.getClosestPoints for k collider pairs of each of m rows: how far apart two shapes are and where their nearest points lie.  The rows are
 * rp_render_states' - src NULL or src->rows NULL: the handle's live envs (m <= N unless row_index is given); else rows of a caller's device buffer in rp_get_state's
 * layout, gathered by src->row_index; src->vis_env is ignored.
 * THE SHAPES are the ones rp_ray_test and the camera meet, WITHOUT MARGINS: a box collider is its exact box, a sphere is centre and radius, an arm or static robot
 * link with a collision hull is the convex hull of its baked vertices, a robot link without one its box.  Any two colliders of one row may be asked, link against link
 * included (which the contact model treats as boxes).  Collider numbers are rp_ray_test's (0 .. n_col - 1, rp_get_collider_dims).
 * pairs: DEVICE int32 [k, 3] = collider a, collider b, group; read by the kernel alone, never on the host.
 * THE RULE: GJK's distance phase on the two support functions (box: the sign of the direction per axis; sphere: its centre, the radius taken off the distance and the
 * witness moved along the normal; hull: the scan of the direction's cell of the support-vertex tables, the lowest vertex number among equals), the simplex in double.
 * The loop is bounded (48 support queries); a pair that reaches the bound reports the best distance it has - an upper bound - with RP_CP_CAPPED OR-ed into its status.
 * PER PAIR (each output may be NULL, not all of them): distance [m, k] float32, point_a / point_b [m, k, 3] (world), normal [m, k, 3] FROM B TOWARD A (the
 * contact convention), status [m, k] int32:
 *   RP_CP_SEPARATED  distance > 0 and point_a - point_b = normal * distance
 *   RP_CP_OVERLAP    GJK ended with the origin inside its simplex or within its zero threshold - the shapes overlap or touch: distance is exactly 0, point_a and
 *                    point_b are both GJK's common point, normal is (0, 0, 0).  PENETRATION DEPTH IS NOT REPORTED (it needs an exact expanding polytope on
 *                    arbitrary hull pairs); the contact model's depths stay the step's business.
 *   RP_CP_FAR        only with max_distance > 0: the gap of the two shapes' world AABBs (the box around a hull is its record's box), a lower bound of the distance,
 *                    exceeds max_distance.  GJK is not run: distance = max_distance, the witnesses and the normal are zero.  max_distance <= 0: no cut.  A pair
 *                    that is not FAR gets the very bits the call without a cut gives it.
 *   RP_CP_SKIPPED    collider a or b outside [0, n_col), a == b, or the row's index outside the buffer: status alone is written, the pair's other outputs KEEP
 *                    WHAT THEY HELD (rp_copy_envs' and rp_render_states' convention for a bad index) - an early exit, not a fault.
 * PER ROW AND GROUP (optional; n_groups = G > 0): group_min [m, G] float32 and group_pair [m, G] int32 = the smallest distance over the group's pairs that are not
 * SKIPPED and the index of that pair, the lowest index among equals; a FAR pair counts with max_distance; an empty group gives +inf and -1; a pair whose group
 * lies outside [0, G) belongs to no group.  Reduced in the same launch, in LDS, no atomics: the result of a scan in pair order, the same bits on every run.
 * COST: per chunk of min(m, max(N, 4096)) rows (rp_render_states' chunks of pose-table slots) two launches on `stream` - k_collider_poses_rows without a sub-goal,
 * k_closest_points (one wave per row, a lane per pair) -; no host wait, no host read of device values; the only allocation is the growth of the pose table.  The call
 * never writes state rows, the contact cache, counters or any table.  It shares the handle's ONE collider-pose table with every call that draws and with rp_ray_test:
 * do not overlap it with such a call on another stream.
 * RP_ERR_ARG (nothing is launched; the message names the cause): m < 1; k outside 1 .. 4096; n_groups outside 0 .. 64; group_min or group_pair given with
 * n_groups == 0; pairs NULL; every output NULL; max_distance not a number; rp_render_states' row-buffer errors (row_stride < 512 or not a multiple of 4, n_rows < 1,
 * row_index NULL with m > n_rows - m > N for live rows). */
enum rp_cp_status { RP_CP_SEPARATED = 0, RP_CP_OVERLAP = 1, RP_CP_FAR = 2, RP_CP_SKIPPED = 3, RP_CP_CAPPED = 4 /* bit */ };
/* the number of colliders: the range of pairs' a and b (the same number rp_get_visuals_dims gives; this one does not speak of visuals) */
int rp_get_collider_dims(rp_handle h, int32_t* n_col);
int rp_closest_points(rp_handle h, const rp_state_rows* src /* NULL or rows NULL: the live envs */, int32_t m,
                      const int32_t* pairs /* DEVICE [k, 3]: collider a, collider b, group */, int32_t k, int32_t n_groups, float max_distance,
                      float* distance /* [m, k] */, float* point_a /* [m, k, 3] */, float* point_b, float* normal,
                      int32_t* status /* [m, k] */, float* group_min /* [m, G] */, int32_t* group_pair /* [m, G] */, void* stream);

/* ---- episodes ended on the device (0.5) ---------------------------------------------------------------------------------------------
 * rp_step_autoreset steps every env as rp_step does (whatever rp_set_fused / rp_set_groups chose) and then resets the envs whose episode ended,
 * on the device: nothing is read back, nothing synchronises, the call returns once the work is enqueued on `stream`.  done[e] (int32 [N]) is
 * the OR of the reasons:
 *   1  the env's episode counter reaches max_episode_steps with this step (when & RP_AR_TIME_LIMIT, max_episode_steps > 0)
 *   2  end_mask[e] != 0 (end_mask [N] uint8, may be NULL)
 *   4  a fault, out.status & 3 (when & RP_AR_FAULT; needs out.status, else RP_ERR_ARG)
 *   8  out.is_success (when & RP_AR_SUCCESS; needs out.is_success, else RP_ERR_ARG)
 * For an env with done != 0: every non-NULL array of final_out gets the row rp_step wrote; the env is then reset with the draws, state record and
 * contact-cache row rp_reset with a mask holding that env would give; out's observation arrays (and the obs_quat | achieved_goal part of out.pack)
 * get the new episode's first observation, while out.reward, out.is_success, out.target_poses and the pack's reward / success columns keep the
 * transition's values and out.status is the step's bits OR the reset's.  Its counter goes to 0; every other env's counter goes up by 1.
 * rp_reset and rp_reset_to set the counters of the envs they reset to 0; rp_step leaves them alone.  The counters are not part of rp_get_state. */
enum rp_autoreset_when { RP_AR_TIME_LIMIT = 1, RP_AR_FAULT = 2, RP_AR_SUCCESS = 4 };
/* max_episode_steps <= 0: no time limit.  Default after rp_create: 0 / RP_AR_FAULT. */
int rp_set_autoreset(rp_handle h, int32_t max_episode_steps, uint32_t when);
/* per-env step counters of the current episode, int32 [N], device pointers */
int rp_get_episode_steps(rp_handle h, int32_t* dst, void* stream);
int rp_set_episode_steps(rp_handle h, const int32_t* src, void* stream);
int rp_step_autoreset(rp_handle h, const float* action, const uint8_t* end_mask /* [N] or NULL */,
                      const rp_out* out, const rp_out* final_out /* may be NULL */, int32_t* done /* [N] */, void* stream);
/* A table of `rows` start vectors o [rows, n_o] (device pointer, the layout rp_reset_to reads; an obs_quat row of the same id is one), copied into
 * library memory on `stream`.  While a table is set, rp_step_autoreset resets every ended env with rp_reset_to semantics from one table row instead of
 * settling: the ended env e gets row (cursor + rank(e)) mod rows, rank(e) = the ended envs with a smaller index in this call, and the cursor then
 * moves on by the number of ends, mod rows.  Everything else follows the rules above (the state record, contact-cache row and outputs are what
 * rp_step followed by rp_reset_to with those rows and a mask of the ended envs would leave, under the autoreset output rules).  rows = 0 (o may be
 * NULL) removes the table: autoreset settles again.  Sets the row cursor to 0.  Synchronises the device before it frees a replaced table; rp_reset and
 * rp_reset_to do not move the cursor, and neither the table nor the cursor is part of rp_get_state.  n_o below what rp_reset_to reads for this id,
 * or rows < 0: RP_ERR_ARG. */
int rp_set_reset_table(rp_handle h, const float* o, int32_t rows, int32_t n_o, void* stream);
/* int32 [N] device pointer: the table row each env's latest rp_step_autoreset started its new episode from; -1 where the env did not end, or ended
 * while no table was set */
int rp_get_reset_rows(rp_handle h, int32_t* dst, void* stream);

/* Per-env dynamics (domain randomisation): every env has one lateral friction per collision object and one mass per free body, float32 device
 * tables friction [N, n_obj] and mass [N, n_free]; rp_create fills them with the baked values.  A contact's friction is the product of its two
 * objects' (at most 10), a torsional row's bound uses the other object's friction (spinning friction stays baked), a free body's mass sets its
 * inverse mass and scales its inertia (uniform density).  The values act from the next substep that builds rows: rp_step in every pipeline, the
 * settle substeps of rp_reset and rp_step_autoreset's resets.  They are parameters, not state: no reset changes them and rp_get_state /
 * rp_set_state do not carry them.  Env indices are the handle's own (0 .. N-1). */
int rp_get_dynamics_dims(rp_handle h, int32_t* n_obj, int32_t* n_free);
/* friction [rows, n_obj] and/or mass [rows, n_free] (NULL = leave that parameter as it is), rows = 1 (broadcast) or N, into every env whose
 * mask byte is non-zero (mask NULL = all).  Enqueued on `stream`; no host wait.  rows not 1 or N, or both arrays NULL: RP_ERR_ARG. */
int rp_set_dynamics(rp_handle h, const float* friction, const float* mass, int32_t rows, const uint8_t* mask, void* stream);
int rp_get_dynamics(rp_handle h, float* friction /* [N, n_obj] or NULL */, float* mass /* [N, n_free] or NULL */, void* stream);

/* Per-env external wrenches (pushes, disturbances, payloads, gravity compensation): every env has, for each of its moving bodies, a force through the body's centre
 * of mass and a torque, both in world coordinates, float32 device table wrench [N, n_body, 6] = fx fy fz tx ty tz.  Bodies in column order: the arm's n_arm links
 * (one per dof, in dof order), the n_free free bodies in the record's order, the n_j1 scene-joint bodies; n_body is their sum.  A free body gains dt f / mass (the env's
 * mass, rp_set_dynamics) and dt R I^-1 R^T t (a rotation-locked body ignores the torque); an arm link's wrench enters the joint torques as -J_com^T f - J_w^T t; a
 * scene joint takes axis . f (prismatic) or axis . t (revolute; the force acts at the joint frame's origin).  The wrench is held: it acts in every substep, from the
 * next substep that builds rows (rp_step in every pipeline, the settle substeps of rp_reset, rp_step_autoreset's resets) until the caller changes it.  It is a
 * parameter, not state: rp_create zeroes it, no reset changes it and rp_get_state / rp_set_state do not carry it.  A zero entry leaves every result bit for bit what it
 * is without a table.  Env indices are the handle's own (0 .. N-1). */
int rp_get_wrench_dims(rp_handle h, int32_t* n_arm, int32_t* n_free, int32_t* n_j1);
/* wrench [rows, n_body, 6], rows = 1 (broadcast) or N, into every env whose mask byte is non-zero (mask NULL = all).  Enqueued on `stream`; no host wait.
 * wrench NULL: zero the masked envs' rows.  rows not 1 or N: RP_ERR_ARG. */
int rp_set_wrench(rp_handle h, const float* wrench, int32_t rows, const uint8_t* mask, void* stream);
int rp_get_wrench(rp_handle h, float* wrench /* [N, n_body, 6] */, void* stream);

/* Per-env gravity and arm-motor gain / strength (a mis-levelled table, an unknown payload, a softer or weaker actuator): every env has a float32 device row
 * act [N, 3 + 2 * n_arm] = gravity[3] (m/s^2, world coordinates), motor_gain[n_arm], motor_strength[n_arm] (both dimensionless, dof order: the arm part of
 * rp_get_wrench's bodies).  The gravity vector stands where (0, 0, -9.8) stood: the arm's base acceleration is -g, a free body's linear velocity gains dt g, a
 * prismatic scene joint dt (axis . g).  An arm motor row asks for the velocity (0.1 * gain_i) (target_i - q_i) / dt and is bounded by -/+ (max impulse_i * strength_i),
 * max impulse_i being what the action wrote into the state record (the record keeps that value).  Scene-joint motors, the Panda's finger gear row and the joint-limit
 * rows do not read the table.  The values act from the next substep that builds rows (rp_step in every pipeline, the settle substeps of rp_reset, rp_step_autoreset's
 * resets).  They are parameters, not state: rp_create writes (0, 0, -9.8), ones and ones, no reset changes them and rp_get_state / rp_set_state do not carry them.
 * With those defaults every result is bit for bit what it is without a table.  Env indices are the handle's own (0 .. N-1). */
int rp_get_actuation_dims(rp_handle h, int32_t* n_arm);
/* gravity [rows, 3], motor_gain [rows, n_arm], motor_strength [rows, n_arm], rows = 1 (broadcast) or N, into every env whose mask byte is non-zero (mask NULL = all).
 * A NULL array leaves that parameter as it is; all three NULL: RP_ERR_ARG.  rows not 1 or N: RP_ERR_ARG.  Enqueued on `stream`; no host wait.  The library does not
 * range-check device values (VecPlayEnv checks host values: |g| <= 50 per component, 0 <= gain <= 10, 0 <= strength <= 10). */
int rp_set_actuation(rp_handle h, const float* gravity, const float* motor_gain, const float* motor_strength, int32_t rows, const uint8_t* mask, void* stream);
int rp_get_actuation(rp_handle h, float* gravity /* [N, 3] or NULL */, float* motor_gain /* [N, n_arm] or NULL */, float* motor_strength /* [N, n_arm] or NULL */,
                     void* stream);

/* Per-env colours, light and background of the camera images (visual domain randomisation): every env has a float32 device row
 * vis [N, 3 * n_col + 8] = colour[n_col][3] (rgb in 0 .. 1 of every collider, in collider order: the index rp_ray_test and the segmentation layer report),
 * light[5] = the direction towards the light dx dy dz (world coordinates, used as it stands: the library does not normalise it), ambient, diffuse, and
 * background[3], the colour of a pixel whose ray meets nothing.  A hit is drawn as colour * (ambient + diffuse * max(0, n . direction)), n the surface normal.
 * rp_render, rp_render_ex and rp_render_layers' rgb read the row of env first_env + i for image i, ghosts included (a ghost has its collider's colour); depth,
 * segmentation and rp_ray_test do not read it.  The button's globe and the dial's grill stay red / white by their state whatever the row says (updateToggles,
 * ENV:469-483: they show state, not appearance).  The values are parameters, not state: the defaults are the colours of the reference's visual shapes, the light
 * (1, -2, 3) / sqrt(14) with ambient 0.45 and diffuse 0.55, and the background (0.82, 0.88, 0.96); no reset, rp_set_state or rp_copy_envs changes them and
 * rp_get_state does not carry them.  With those defaults every image is byte for byte what it is without a table.  The table (up to 800 bytes per env) does not
 * exist until the first rp_set_visuals or rp_get_visuals, which allocates it and fills it with the defaults on the call's stream; rp_destroy frees it.  Env
 * indices are the handle's own (0 .. N-1). */
int rp_get_visuals_dims(rp_handle h, int32_t* n_col);
/* colour [rows, n_col, 3], light [rows, 5], background [rows, 3], rows = 1 (broadcast) or N, into every env whose mask byte is non-zero (mask NULL = all).
 * A NULL array leaves that part as it is; all three NULL: RP_ERR_ARG.  rows not 1 or N: RP_ERR_ARG.  Enqueued on `stream`; no host wait, no host read of device
 * values.  The library does not range-check device values (VecPlayEnv checks host values: colour and background in [0, 1], ambient and diffuse >= 0, a direction
 * of non-zero length, which it normalises and keeps to seven decimals, so that (1, -2, 3) is the default direction bit for bit). */
int rp_set_visuals(rp_handle h, const float* colour, const float* light, const float* background, int32_t rows, const uint8_t* mask, void* stream);
int rp_get_visuals(rp_handle h, float* colour /* [N, n_col, 3] or NULL */, float* light /* [N, 5] or NULL */, float* background /* [N, 3] or NULL */,
                   void* stream);

/* Per-env joint and body state by column (a drawer half open, a thrown block, an arm at a joint vector without IK; the reference's resetJointState,
 * resetBasePositionAndOrientation, resetBaseVelocity and their getters, ENV:519-603): the kinematic words of the state record as two float32 tables, with
 * n_arm, n_free, n_j1 of rp_get_wrench_dims,
 *   pos [N, n_pos], n_pos = n_arm + 7 * n_free + n_j1: arm q[n_arm] (dof order), per free body x y z qx qy qz qw (record order), scene-joint q[n_j1]
 *   vel [N, n_vel], n_vel = n_arm + 6 * n_free + n_j1: arm qd, per free body vx vy vz wx wy wz (world), scene-joint qd
 * - the order of the oracle's rpo_get_state vector with positions and velocities split.  rp_set_kinematics writes exactly those words, verbatim (a quaternion is not
 * normalised; VecPlayEnv checks host values), for every env whose mask byte is non-zero (mask NULL = all); rows = 1 (broadcast) or N; a NULL array leaves that half as it
 * is.  Nothing else changes: motor mode / target / max impulse, goal, quaternion sign memory, RNG counter, status, episode counter and the dynamics, wrench and
 * actuation tables stay.  The contact-cache row stays too, as rp_reset_to leaves it: the next substep's refresh drops the points beyond their breaking threshold.  With
 * RP_KIN_CLEAR_CONTACTS the masked envs' cache rows are zeroed (a state without contact history); under RP_CFG_STATELESS_CONTACTS the flag does nothing.  Enqueued on
 * `stream`; no host wait, no host read of device values.  Both arrays NULL, rows not 1 or N, unknown flag bits: RP_ERR_ARG. */
enum rp_kin_flags { RP_KIN_CLEAR_CONTACTS = 1 };
int rp_get_kinematics(rp_handle h, float* pos /* [N, n_pos] or NULL */, float* vel /* [N, n_vel] or NULL */, void* stream);
int rp_set_kinematics(rp_handle h, const float* pos, const float* vel, int32_t rows, const uint8_t* mask, uint32_t flags, void* stream);

/* Envs cloned on the device (CEM-MPC rollouts from one state, population-based training, particle resampling): every env e whose mask byte is non-zero (mask NULL = all)
 * takes the whole state row of env src[e] (int32 [N], device pointer) AS IT WAS BEFORE THE CALL - the state record and, unless RP_CFG_STATELESS_CONTACTS, the
 * contact-cache row: what rp_get_state, a gather of the rows by src and rp_set_state would leave.  Gather semantics: any src is served (permutations, cycles,
 * many-to-one, identity).  With RP_COPY_EPISODE_STEPS the env also takes that env's episode counter.  An env whose src[e] is outside [0, N) is left unchanged.  The
 * dynamics, wrench, actuation and visuals tables, the reset table and its cursor are not copied.  Staging: every row is first copied into a buffer of the handle's own, one extra
 * copy of the rows (rp_state_bytes + 4 bytes per env), allocated by the first call and freed by rp_destroy - not the row workspace, so rp_debug_row_counts still sees the
 * latest substep.  Two launches on `stream`; no host wait.  The call reads and writes the state rows and shares the one staging buffer: do not overlap it with rp_step,
 * rp_reset or another rp_copy_envs of the same handle on another stream.  src NULL, unknown flag bits: RP_ERR_ARG. */
enum rp_copy_flags { RP_COPY_EPISODE_STEPS = 1 };
int rp_copy_envs(rp_handle h, const int32_t* src /* [N] */, const uint8_t* mask, uint32_t flags, void* stream);

int rp_get_timers(rp_handle h, rp_timers* t);
/* on = number of rp_step calls to keep per-launch timings for (a ring); 0 disables */
int rp_enable_timers(rp_handle h, int32_t on);
const char* rp_last_error(rp_handle h);
const char* rp_version(void);

#ifdef __cplusplus
}
#endif
#endif
