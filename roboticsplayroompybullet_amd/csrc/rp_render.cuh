/* rp_render.cuh — headless camera images and batched ray queries over the collider tables.
 *
 * The reference renders obs['img'] with PyBullet's OpenGL rasteriser (environments.py:21-30, 841-845: getCameraImage(200, 200,
 * viewMatrix, projectionMatrix), fixed camera; gripper camera environments.py:33-49) and queries one ray per step for
 * gripper_proprioception (environments.py:720-743, rayTest).  Here both are ray casts against the SAME shapes the contact model uses - boxes, spheres and, for the arm's
 * links, the convex hulls of their collision meshes (round 5: until then their boxes) - the only geometry the library holds - with the colours of the reference's visual shapes (scenes.py rgbaColor, URDF
 * materials; the button's globe and the dial's grill recoloured as updateToggles does, environments.py:469-483), flat Lambert shading,
 * no textures, no shadows (the reference passes shadow=0).  Sub-goal visualisation (environments.py:606-690) = the same bodies drawn a
 * second time, half transparent, at the poses a sub-goal vector names.
 *
 *   k_collider_poses   one wave per env: FK -> world pose, half extents, colour of every collider (+ the ghosts of a sub-goal); the colour from the env's visuals row
 *                      where rp_set_visuals made a table
 *   k_render_layers    a 16 x 16 pixel tile per block, the tile's shortlist of records in LDS, nearest hit per pixel: colour, depth and segmentation; per-env
 *                      cameras (rp_render, rp_render_ex: the colour alone; rp_render_layers)
 *   k_render_views     the tiles of up to four views of the same envs in one launch, behind one k_collider_poses (rp_set_image_views)
 *                      all three as <SEL = true> too: the envs a device array selects (rp_set_image_obs: the ended envs' terminal frames, a masked reset's images)
 *   k_collider_poses_rows, k_render_states   the same two for state rows that are not the handle's own: rows of a caller's buffer, gathered by an index, each drawn
 *                      with a named row of the visuals table, a sub-goal as ghosts or SOLID (rp_render_states)
 *   k_point_cloud      behind a draw: the hits of an env's depth + segmentation layers compacted in scan order into a fixed number of points, evenly subsampled
 *                      (rp_render_points, rp_set_image_points); <SEL = true> as above
 *   k_ray_test         K rays per env against the same table: hit fraction, position, normal, collider, Bullet link index */
#pragma once

#define RC_STRIDE 20          /* floats per collider record: R9 p3 he3 rgb3 type|flags link */
#define RC_MAX (2 * RP_MAX_COL)
#define RC_GHOST 0x100        /* flag in the type word: drawn half transparent, ignored by rp_ray_test */
#define RC_HULL 0x200         /* flag in the type word: an arm link - the record's box is the box AROUND its collision hull, the shape is the hull (DevModel.hpl: its face planes) */

struct RpCamera { float eye[3], fwd[3], right[3], up[3]; float tan_half_fov, aspect; int mode; };   /* mode 1: at the EE link (gripper camera) */

/* per-env visuals (rp_set_visuals): a row of the table is colour[n_col][3], then light = direction towards the light[3] ambient diffuse, then background[3].  The kernels
 * take a null table as a table of default rows - the baked colours (DevModel.col_rgb) and the literals below - and do the same arithmetic either way */
#define VIS_TAIL 8            /* floats behind the colours: light 5, background 3 */
#define VIS_LIGHT_X 0.2672612f
#define VIS_LIGHT_Y -0.5345225f
#define VIS_LIGHT_Z 0.8017837f      /* (1, -2, 3) / sqrt(14) */
#define VIS_AMBIENT 0.45f
#define VIS_DIFFUSE 0.55f
#define VIS_BG_R 0.82f
#define VIS_BG_G 0.88f
#define VIS_BG_B 0.96f

/* a subset of the envs that the DEVICE names (rp_set_image_obs: rp_step_autoreset's done[N] for the terminal frames, a reset's mask[N]): env is drawn unless its word of
 * sel32 or its byte of sel8 is 0; both indexed by env, each may be null.  The two kernels that take a selection are templates on SEL: SEL = false never looks at the
 * pointers and is, instruction for instruction, the kernel without a selection (with the test compiled in and null pointers the compiler laid out the ray loop's branches
 * another way, and a draw of all envs cost 0.5 % more: profiles/image_obs_rate.txt); the host launches SEL = true only where a pointer is given. */
__device__ __forceinline__ bool rc_selected(const int* __restrict__ sel32, const unsigned char* __restrict__ sel8, int env) {
  return !(sel32 && sel32[env] == 0) && !(sel8 && sel8[env] == 0);
}

/* world pose of every collider of env `first + blockIdx.x` into tab[blockIdx.x][RC_MAX][RC_STRIDE]; cnt[blockIdx.x] = records written.
 * sub_goal (may be null): [num][n_ag] achieved-goal vectors to visualise as ghosts (objects, drawer, door, button, dial).
 * ghost_arm (may be null): [num][8] = EE position, orientation quaternion, gripper: the ghost ARM of visualise_sub_goal's 'controllable_achieved_goal' /
 * 'full_positional_state' (environments.py:623-637, 671-674: reset_arm(ghost_arm, sub_goal, from_init=False) = the arm at its rest pose, one default IK call of 20
 * iterations towards the pose, joints [0:6] taken - reset_arm_goal_obs' arithmetic), drawn half transparent like the other ghosts.
 * vis (may be null): the visuals table [N][3 n_col + VIS_TAIL] of the whole handle; env `first + blockIdx.x` takes its colliders' colours from its own row, ghosts included,
 * null = the baked colours.  The toggles' red / white (updateToggles) shows state, not appearance, and stands on top of either.
 * sel32, sel8 (each may be null): the selection (rc_selected); the block of an unselected env leaves at the top, before the state load and any barrier, and writes
 * nothing: its slot of tab / cnt / ee_pose keeps what it held. */
template <bool SEL>
__global__ void __launch_bounds__(64) k_collider_poses(const DevModel* __restrict__ m, const float* __restrict__ state, int first, int num,
                                                       float* __restrict__ tab, int* __restrict__ cnt, const float* __restrict__ sub_goal,
                                                       float* __restrict__ ee_pose, const float* __restrict__ ghost_arm, const float* __restrict__ vis,
                                                       const int* __restrict__ sel32, const unsigned char* __restrict__ sel8) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= num) return;
  const int env = first + slot;
  if (SEL && !rc_selected(sel32, sel8, env)) return;      /* block-uniform: the whole wave leaves */
  __shared__ EnvLds L;
  const int srow = env, venv = env;      /* the env's own state row and its own visuals row */
  constexpr bool SOLID = false;
#include "rp_collider_poses_body.inc"
}

/* rp_render_states: the poses of one chunk of images, slot = the image's place in the chunk.  Image `slot` draws row row_index[slot] of `rows` (row_index null: row
 * base + slot; the host hands row_index, vis_env and goal in already moved to the chunk's first image) - row_floats floats from one row to the next, the first
 * RP_REC_FLOATS of a row are the state record - with the colours of row vis_env[slot] of the handle's visuals table `vis`; a null vis or vis_env, or an entry outside
 * [0, n_envs), gives the baked colours.  A row outside [0, n_rows) is an UNWRITTEN image: the block leaves here, before it reads the row and before any barrier, and
 * writes nothing (k_render_states makes the same test and never reads this slot of tab / cnt / ee_pose).  goal (may be null): [num][n_ag], k_collider_poses' sub_goal;
 * SOLID: rp_collider_poses_body.inc.  Nothing but tab / cnt / ee_pose is written: the handle's state is read, at most. */
template <bool SOLID>
__global__ void __launch_bounds__(64) k_collider_poses_rows(const DevModel* __restrict__ m, const float* __restrict__ rows, size_t row_floats, int n_rows,
                                                            const int* __restrict__ row_index, int base, int num, float* __restrict__ tab, int* __restrict__ cnt,
                                                            const float* __restrict__ goal, float* __restrict__ ee_pose, const float* __restrict__ vis_tab,
                                                            const int* __restrict__ vis_env, int n_envs) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= num) return;
  const int row = row_index ? row_index[slot] : base + slot;
  if (row < 0 || row >= n_rows) return;                   /* block-uniform: the whole wave leaves */
  const int ve = vis_env ? vis_env[slot] : -1;
  const bool own = vis_tab && ve >= 0 && ve < n_envs;
  __shared__ EnvLds L;
  const float* state = rows + (size_t)row * row_floats;      /* the body's names: the record is row 0 from here, no ghost arm, the named visuals row */
  const float* sub_goal = goal;
  const float* ghost_arm = nullptr;
  const float* vis = own ? vis_tab : nullptr;
  const int srow = 0, venv = own ? ve : 0;
#include "rp_collider_poses_body.inc"
}

/* ray o + t d, t in [0, tmax], against a box (R, p, he): entry parameter and the face normal, world frame.  A ray that starts
 * inside reports no hit (Bullet's convex ray test). */
__device__ __forceinline__ bool rc_ray_box(const float* rec, V3 o, V3 d, float tmax, float& t_hit, V3& n_hit) {
  const M3 R = ldm3(rec);
  const V3 ol = tmulv(R, o - ld3(rec + 9)), dl = tmulv(R, d);
  const float o3[3] = {ol.x, ol.y, ol.z}, d3[3] = {dl.x, dl.y, dl.z}, h3[3] = {rec[12], rec[13], rec[14]};
  if (fabsf(o3[0]) <= h3[0] && fabsf(o3[1]) <= h3[1] && fabsf(o3[2]) <= h3[2]) return false;
  float tmin = 0.f, tm = tmax; int axis = 0; float sgn = 0.f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (fabsf(d3[k]) < 1e-12f) { if (fabsf(o3[k]) > h3[k]) return false; continue; }
    float t1 = (-h3[k] - o3[k]) / d3[k], t2 = (h3[k] - o3[k]) / d3[k], s = -1.f;
    if (t1 > t2) { float w = t1; t1 = t2; t2 = w; s = 1.f; }
    if (t1 > tmin) { tmin = t1; axis = k; sgn = s; }
    tm = fminf(tm, t2);
    if (tmin > tm) return false;
  }
  t_hit = tmin;
  n_hit = col(R, axis) * sgn;
  return true;
}
/* ... against an arm link: the convex hull of its collision mesh - what the link collides as (rp_kernels.cuh hull_item16) - by clipping the ray against the hull's face
 * planes (collider frame, n . x + w <= 0 inside), after the box around the hull, which most rays miss.  The reference draws the links' visual meshes; rounds 3 and 4 drew the
 * boxes.  A ray that starts inside reports no hit, like the box's. */
__device__ __forceinline__ bool rc_ray_hull(const float* rec, const float4* __restrict__ pl, int npl, V3 o, V3 d, float tmax, float& t_hit, V3& n_hit) {
  const M3 R = ldm3(rec);
  const V3 ol = tmulv(R, o - ld3(rec + 9)), dl = tmulv(R, d);
  {      /* the box around the hull as a SLAB-OVERLAP cull only: a ray that starts inside the box but outside the hull (the gripper camera at the EE link, a ray cast from
          * beside the arm: the links' boxes are much larger than their hulls) still meets the planes below - rc_ray_box's "starts inside = no hit" is about the hull */
    const float o3[3] = {ol.x, ol.y, ol.z}, d3[3] = {dl.x, dl.y, dl.z}, h3[3] = {rec[12], rec[13], rec[14]};
    float tmin = 0.f, tm = tmax;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (fabsf(d3[k]) < 1e-12f) { if (fabsf(o3[k]) > h3[k]) return false; continue; }
      float t1 = (-h3[k] - o3[k]) / d3[k], t2 = (h3[k] - o3[k]) / d3[k];
      if (t1 > t2) { const float w = t1; t1 = t2; t2 = w; }
      tmin = fmaxf(tmin, t1); tm = fminf(tm, t2);
      if (tmin > tm) return false;
    }
  }
  float t_in = 0.f, t_out = tmax; V3 nl = mk3(0, 0, 0); bool entered = false;
  for (int k = 0; k < npl; k++) {
    const float4 p = pl[k];
    const float den = p.x * dl.x + p.y * dl.y + p.z * dl.z, num = -(p.x * ol.x + p.y * ol.y + p.z * ol.z + p.w);
    if (fabsf(den) < 1e-12f) { if (num < 0.f) return false; continue; }      /* parallel to the plane: outside it = a miss */
    const float t = num / den;
    if (den < 0.f) { if (t > t_in) { t_in = t; nl = mk3(p.x, p.y, p.z); entered = true; } }
    else t_out = fminf(t_out, t);
    if (t_in > t_out) return false;
  }
  if (!entered) return false;
  t_hit = t_in;
  n_hit = mulv(R, nl);
  return true;
}
__device__ __forceinline__ bool rc_ray_sphere(const float* rec, V3 o, V3 d, float tmax, float& t_hit, V3& n_hit) {
  const V3 c = ld3(rec + 9), oc = o - c;
  const float r = rec[12], a = dot(d, d), b = 2.f * dot(oc, d), cc = dot(oc, oc) - r * r;
  if (cc < 0.f) return false;
  const float disc = b * b - 4.f * a * cc;
  if (disc < 0.f) return false;
  const float t = (-b - sqrtf(disc)) / (2.f * a);
  if (t < 0.f || t > tmax) return false;
  t_hit = t;
  n_hit = (oc + d * t) * (1.f / r);
  return true;
}
/* ... against a collider record, as the shape its type word names: an arm link's hull, a box, a sphere */
__device__ __forceinline__ bool rc_hit(const DevModel* __restrict__ m, const float* rec, V3 o, V3 d, float tmax, float& t, V3& n) {
  const int tw = __float_as_int(rec[18]), ci = __float_as_int(rec[19]) & 0xFF;
  return (tw & RC_HULL) ? rc_ray_hull(rec, (const float4*)m->hpl + m->hpl_off[ci], m->hpl_cnt[ci], o, d, tmax, t, n)
                        : ((tw & 0xFF) == 0 ? rc_ray_box(rec, o, d, tmax, t, n) : rc_ray_sphere(rec, o, d, tmax, t, n));
}

/* gripper_camera (environments.py:33-49) from the EE link's rotation R: ori = the link's Euler angles + (0, -pi / 2, 0), rot = the matrix of ori's quaternion, camera
 * vector = rot (1, 0, 0), up vector = rot (0, 0, 1), then computeViewMatrix(pos, pos + camera vector, up vector): f = the camera vector, s = f x up normalised, u = s x f.
 * With (roll, pitch, yaw) the link's angles this is f = Rz(yaw) Ry(pitch) z and u = Rz(yaw) Ry(pitch) (-cos roll, -sin roll, 0) - NOT a fixed rotation of the link frame: it
 * is the link's (-z, +x) only at roll = pi (what rounds 3 to 6 drew for every pose) and (+z, -x) at roll = 0, the reset pose.  The operations are the reference's own, one by
 * one with the library's conversions; tests/golden/render_parent_checksums.json pins their bits. */
__device__ __forceinline__ void rc_gripper_basis(const M3& R, V3& fwd, V3& right, V3& up) {
  const Q4 q = m3_to_quat(R);
  const V3 e = euler_from_quat(q.x, q.y, q.z, q.w);
  const M3 rot = quat_to_m3(quat_from_euler(e.x, e.y - 0.5f * RP_PI_F, e.z));
  const V3 f = col(rot, 0), u0 = col(rot, 2);
  fwd = f * (1.f / norm(f));
  const V3 s = cross(fwd, u0);
  right = s * (1.f / norm(s));
  up = cross(right, fwd);
}

/* the view of env slot `slot` of a launch into V[0 .. 13] = eye, fwd, right, up, tan_half_fov, aspect (one thread; V in LDS): from the env's row of cam_rows with
 * device_camera's operations (rp_playroom.hip) in double, else from the launch's RpCamera, for the gripper camera (mode 1) at the env's EE pose.  rc_draw_tile and
 * k_point_cloud both build their view here, so a point is unprojected along the very ray its pixel was cast along. */
__device__ __forceinline__ void rc_view_basis(const RpCamera& cam, const float* __restrict__ cam_rows, const float* __restrict__ ee_pose, int slot, float* V) {
  if (cam_rows) {      /* device_camera (rp_playroom.hip), operation by operation */
    const float* c = cam_rows + 11 * (size_t)slot;
    double f[3], u[3], s[3], nn = 0;
    for (int k = 0; k < 3; k++) { f[k] = c[3 + k] - c[k]; nn += f[k] * f[k]; }
    nn = sqrt(nn > 0 ? nn : 1);
    for (int k = 0; k < 3; k++) f[k] /= nn;
    s[0] = f[1] * c[8] - f[2] * c[7]; s[1] = f[2] * c[6] - f[0] * c[8]; s[2] = f[0] * c[7] - f[1] * c[6];
    nn = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); nn = nn > 0 ? nn : 1;
    for (int k = 0; k < 3; k++) s[k] /= nn;
    u[0] = s[1] * f[2] - s[2] * f[1]; u[1] = s[2] * f[0] - s[0] * f[2]; u[2] = s[0] * f[1] - s[1] * f[0];
    for (int k = 0; k < 3; k++) { V[k] = c[k]; V[3 + k] = (float)f[k]; V[6 + k] = (float)s[k]; V[9 + k] = (float)u[k]; }
    V[12] = (float)tan(0.5 * c[9] * 0.01745329251994329547); V[13] = c[10];
  } else {
    V3 eye = ld3(cam.eye), fwd = ld3(cam.fwd), right = ld3(cam.right), up = ld3(cam.up);
    if (cam.mode == 1) {       /* gripper_camera (environments.py:33-49): at the EE link, the reference's basis from the link's Euler angles */
      const float* e = ee_pose + 12 * slot;
      eye = ld3(e);
      rc_gripper_basis(ldm3(e + 3), fwd, right, up);
    }
    st3(V, eye); st3(V + 3, fwd); st3(V + 6, right); st3(V + 9, up);
    V[12] = cam.tan_half_fov; V[13] = cam.aspect;
  }
}

/* rp_render, rp_render_ex (obs['img'], environments.py:841-845: the colour alone) and rp_render_layers: colour, depth and segmentation of getCameraImage in one pass, a
 * 16 x 16 pixel tile per block, one thread per pixel, row 0 = top of the image, uint8 rgb.
 *
 * The block first builds its view (thread 0: the camera's basis - from the launch's RpCamera, from the EE pose for the gripper camera, or from the env's row of
 * cam_rows with device_camera's operations in double) and then the tile's SHORTLIST: one lane per collider record tests the record's bounding sphere (centre p, radius |he|
 * for a box or the box around a hull, r for a sphere) against the four side planes of the tile's frustum - the pyramid with the eye as apex through the centres of the
 * tile's outermost pixels, whose nx / ny are computed by the very expression the pixels use, so every pixel-centre ray of the tile lies inside it.  A record is dropped only
 * when its sphere lies wholly outside one of the planes by more than a pad of 1e-3 of the distances involved (fp32 rounds at 6e-8; the basis is orthonormal to about 1e-6):
 * then no pixel-centre ray of the tile can meet it, and dropping it cannot change a pixel.  Ballots and a prefix count over the four waves compact the survivors into LDS in
 * ASCENDING record order, so that the lowest record still wins a tie as it does on the whole table.  Each pixel then walks the shortlist: its ray, rc_hit per record, flat Lambert
 * shading, the ghosts blended at 0.5.  cull == 0 (rp_debug_render_cull): every record is on every tile's list.
 *
 * depth: the nearest NON-ghost hit as eye-space z = t (d . fwd) - t the hit parameter of the winning record, for a sphere re-evaluated in a well-conditioned form (below; which
 * record wins, and the colour, stay with rc_ray_sphere's t) -; RP_DEPTH_BUFFER far (z - near) / (z (far - near)) clamped to [0, 1], 1 on a miss; RP_DEPTH_METRES z, far on
 * a miss.  seg: collider | (link + 1) << 24 of that hit (rp_ray_test's collider and link), -1 on a miss.  Ghosts tint rgb only.
 *
 * vis (may be null): the handle's visuals table; thread 0 stages the light and the background of env `first + slot` behind the camera in V[] (null: the literals), and the
 * shading and the miss colour read them there.  The direction is used as it stands (not normalised).  Depth and segmentation do not read the table.
 *
 * sel32, sel8 (each may be null): k_collider_poses' selection, by env `first + slot`; every tile's block of an unselected env leaves before the view is built - all 256
 * threads, ahead of the first barrier - and the env's rows of rgb / depth / seg keep what they held. */
static_assert(RC_MAX <= 256, "k_render_layers: one lane per record");
/* one tile of one env, everything behind the kernels' split of blockIdx.x: the view, the shortlist, the pixels (the comment above).  k_render_layers and k_render_views
 * both draw through it, so a row is the same bytes whichever kernel wrote it; inlined, each kernel owns its copy of the LDS arrays. */
__device__ __forceinline__ void rc_draw_tile(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, const RpCamera& cam,
                                             const float* __restrict__ cam_rows, const float* __restrict__ ee_pose, int width, int height, int cull, float near_plane,
                                             float far_plane, int metres, unsigned char* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ seg,
                                             const float* __restrict__ vis, int first, int slot, int tile, int tiles_x) {
  __shared__ float T[RC_MAX * RC_STRIDE];      /* the shortlist's records, compacted */
  __shared__ float V[14 + VIS_TAIL];           /* eye, fwd, right, up, tan_half_fov, aspect; light direction, ambient, diffuse, background */
  __shared__ int list[RC_MAX];
  __shared__ int wcnt[4];
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    rc_view_basis(cam, cam_rows, ee_pose, slot, V);
    if (vis) {
      const float* lb = vis + (size_t)(first + slot) * (3 * m->n_col + VIS_TAIL) + 3 * m->n_col;
      for (int k = 0; k < VIS_TAIL; k++) V[14 + k] = lb[k];
    } else {
      V[14] = VIS_LIGHT_X; V[15] = VIS_LIGHT_Y; V[16] = VIS_LIGHT_Z; V[17] = VIS_AMBIENT; V[18] = VIS_DIFFUSE;
      V[19] = VIS_BG_R; V[20] = VIS_BG_G; V[21] = VIS_BG_B;
    }
  }
  __syncthreads();
  const V3 eye = ld3(V), fwd = ld3(V + 3), right = ld3(V + 6), up = ld3(V + 9);
  const float thf = V[12], aspect = V[13];
  const int n = min(cnt[slot], RC_MAX);
  const float* G = tab + (size_t)slot * RC_MAX * RC_STRIDE;
  bool keep = tid < n;
  if (keep && cull) {
    const float* rec = G + tid * RC_STRIDE;
    const V3 q = ld3(rec + 9) - eye, he = ld3(rec + 12);
    const int tw = __float_as_int(rec[18]);
    const float r = (!(tw & RC_HULL) && (tw & 0xFF) != 0) ? he.x : norm(he);      /* a sphere's radius; the corner of a box or of the box around a hull */
    const float qx = dot(q, right), qy = dot(q, up), qz = dot(q, fwd);
    const float pad = r + 1e-3f * (r + fabsf(qx) + fabsf(qy) + fabsf(qz)) + 1e-4f;
    const int x1 = min(16 * tx + 15, width - 1), y1 = min(16 * ty + 15, height - 1);
    const float nxa = (2.f * (16 * tx + 0.5f) / width - 1.f) * thf * aspect, nxb = (2.f * (x1 + 0.5f) / width - 1.f) * thf * aspect;      /* left <= right */
    const float nya = (1.f - 2.f * (16 * ty + 0.5f) / height) * thf, nyb = (1.f - 2.f * (y1 + 0.5f) / height) * thf;                        /* top >= bottom */
    keep = !(nxa * qz - qx > pad * sqrtf(1.f + nxa * nxa) || qx - nxb * qz > pad * sqrtf(1.f + nxb * nxb) ||
             qy - nya * qz > pad * sqrtf(1.f + nya * nya) || nyb * qz - qy > pad * sqrtf(1.f + nyb * nyb));
  }
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, nl = 0;
  for (int w = 0; w < 4; w++) { const int c = wcnt[w]; before += w < wave ? c : 0; nl += c; }
  if (keep) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
  __syncthreads();
  for (int i = tid; i < nl * RC_STRIDE; i += 256) { const int r = i / RC_STRIDE; T[i] = G[list[r] * RC_STRIDE + (i - r * RC_STRIDE)]; }
  __syncthreads();
  const int px = 16 * tx + (tid & 15), py = 16 * ty + (tid >> 4);
  if (px >= width || py >= height) return;
  const float nx = (2.f * (px + 0.5f) / width - 1.f) * thf * aspect, ny = (1.f - 2.f * (py + 0.5f) / height) * thf;
  V3 d = fwd + right * nx + up * ny;
  d = d * (1.f / norm(d));
  const float far = 10.f;
  float best = far, gbest = far; V3 bn = mk3(0, 0, 1), gn = bn; int bi = -1, gi = -1;
  for (int c = 0; c < nl; c++) {
    const float* rec = &T[c * RC_STRIDE];
    float t; V3 nn;
    if (!rc_hit(m, rec, eye, d, far, t, nn)) continue;
    if (__float_as_int(rec[18]) & RC_GHOST) { if (t < gbest) { gbest = t; gn = nn; gi = c; } }
    else if (t < best) { best = t; bn = nn; bi = c; }
  }
  const size_t pix = (size_t)slot * width * height + (size_t)py * width + px;
  if (rgb) {
    const V3 light = ld3(V + 14);                                         /* the env's directional light (default (1, -2, 3) / sqrt(14)) */
    const float ambient = V[17], diffuse = V[18];
    auto shade = [&](int c, V3 nn) {
      const float* rec = &T[c * RC_STRIDE];
      const float k = ambient + diffuse * fmaxf(0.f, dot(nn, light));
      return mk3(rec[15] * k, rec[16] * k, rec[17] * k);
    };
    V3 colr = ld3(V + 19);                                                /* background */
    if (bi >= 0) colr = shade(bi, bn);
    if (gi >= 0 && gbest < best) colr = colr * 0.5f + shade(gi, gn) * 0.5f;  /* the ghosts are drawn with alpha 0.5 (environments.py:650) */
    unsigned char* o = rgb + pix * 3;
    o[0] = (unsigned char)(fminf(fmaxf(colr.x, 0.f), 1.f) * 255.f + 0.5f);
    o[1] = (unsigned char)(fminf(fmaxf(colr.y, 0.f), 1.f) * 255.f + 0.5f);
    o[2] = (unsigned char)(fminf(fmaxf(colr.z, 0.f), 1.f) * 255.f + 0.5f);
  }
  if (depth) {
    float tz = best;
    if (bi >= 0) {      /* a sphere's hit parameter again, well conditioned: rc_ray_sphere's b b - 4 a c cancels at a grazing ray (to 1.5e-7 out of two terms near 6 on the button's globe,
                         * 3e-4 m of depth); through the point of closest approach the same root is t_c - sqrt(r r - |o - c + t_c d|^2), whose terms are of the size of r */
      const float* rec = &T[bi * RC_STRIDE];
      const int tw = __float_as_int(rec[18]);
      if (!(tw & RC_HULL) && (tw & 0xFF) != 0) {
        const V3 oc = eye - ld3(rec + 9);
        const float tc = -dot(oc, d);
        const V3 perp = oc + d * tc;
        tz = tc - sqrtf(fmaxf(rec[12] * rec[12] - dot(perp, perp), 0.f));
      }
    }
    const float z = tz * dot(d, fwd);
    depth[pix] = bi < 0 ? (metres ? far_plane : 1.f) : (metres ? z : fminf(fmaxf(far_plane * (z - near_plane) / (z * (far_plane - near_plane)), 0.f), 1.f));
  }
  if (seg) {
    const int id = bi >= 0 ? __float_as_int(T[bi * RC_STRIDE + 19]) : 0;
    seg[pix] = bi >= 0 ? ((id & 0xFF) | (((id >> 8) + 1) << 24)) : -1;
  }
}


template <bool SEL>
__global__ void __launch_bounds__(256) k_render_layers(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, int num, RpCamera cam,
                                                       const float* __restrict__ cam_rows, const float* __restrict__ ee_pose, int width, int height, int cull,
                                                       float near_plane, float far_plane, int metres, unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                                       int* __restrict__ seg, const float* __restrict__ vis, int first, const int* __restrict__ sel32,
                                                       const unsigned char* __restrict__ sel8) {
  const int tiles_x = (width + 15) >> 4, tiles = tiles_x * ((height + 15) >> 4);
  /* tile-major: consecutive blocks are the SAME tile of consecutive envs.  Blocks go to the eight XCDs round robin; env-major, with a tile count that is a multiple of
   * eight (64 x 64: 16), the few tiles that hold the arm - whose hulls cost a ray hundreds of plane tests - would always land on the same XCDs */
  const int tile = blockIdx.x / num, slot = blockIdx.x - tile * num;
  if (tile >= tiles) return;
  if (SEL && !rc_selected(sel32, sel8, first + slot)) return;
  rc_draw_tile(m, tab, cnt, cam, cam_rows, ee_pose, width, height, cull, near_plane, far_plane, metres, rgb, depth, seg, vis, first, slot, tile, tiles_x);
}

/* rp_render_states: k_render_layers for one chunk of images behind k_collider_poses_rows, the same tile-major block numbering.  The light and the background come from
 * row vis_env[slot] of the visuals table (a null vis or vis_env, or an entry outside [0, n_envs): the literals, as under a null table); rc_draw_tile reads row
 * first + slot, so it is handed first = that row - slot, or a null table.  Every tile's block of an unwritten image (k_collider_poses_rows' test of the row) leaves
 * ahead of the first barrier and the image's rows of rgb / depth / seg keep what they held.  The pixels are rc_draw_tile's: the bytes of k_render_layers. */
__global__ void __launch_bounds__(256) k_render_states(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, int num, RpCamera cam,
                                                       const float* __restrict__ cam_rows, const float* __restrict__ ee_pose, int width, int height, int cull,
                                                       float near_plane, float far_plane, int metres, unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                                       int* __restrict__ seg, const float* __restrict__ vis, const int* __restrict__ vis_env, int n_envs,
                                                       const int* __restrict__ row_index, int base, int n_rows) {
  const int tiles_x = (width + 15) >> 4, tiles = tiles_x * ((height + 15) >> 4);
  const int tile = blockIdx.x / num, slot = blockIdx.x - tile * num;
  if (tile >= tiles) return;
  const int row = row_index ? row_index[slot] : base + slot;
  if (row < 0 || row >= n_rows) return;
  const int ve = vis_env ? vis_env[slot] : -1;
  const bool own = vis && ve >= 0 && ve < n_envs;
  rc_draw_tile(m, tab, cnt, cam, cam_rows, ee_pose, width, height, cull, near_plane, far_plane, metres, rgb, depth, seg, own ? vis : nullptr, own ? ve - slot : 0, slot, tile,
               tiles_x);
}

/* rp_set_image_views: up to RC_MAX_VIEWS views of the same envs in ONE launch, behind one k_collider_poses (the poses and ee_pose do not depend on the camera).  The
 * table travels by value in the kernel arguments; the host builds it once, at the set call.  tile0: the view's first tile in the list of all views' tiles, one behind
 * the other; every view covers the same `num` envs, slot = env (first = 0). */
#define RC_MAX_VIEWS 4
struct RpViewEntry {
  RpCamera cam; const float* cam_rows;
  int width, height, tiles_x, tiles, tile0;
  float near_plane, far_plane; int metres;
  unsigned char* rgb; float* depth; int* seg;
};
struct RpViewTable { RpViewEntry v[RC_MAX_VIEWS]; };

/* Block numbering as k_render_layers', tile-major over the CONCATENATED tile list: consecutive blocks are the same tile of the same view for consecutive envs, and the
 * long tiles of one view (the arm's) run beside the short ones of another instead of ending a launch of their own.  The view of a block is found by at most three
 * block-uniform compares; an unselected env's block leaves right after the split, before the table is read.  The rest is rc_draw_tile: the bytes of
 * k_render_layers(that view's arguments). */
template <bool SEL>
__global__ void __launch_bounds__(256) k_render_views(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, int num,
                                                      const RpViewTable vt, int n_views, int total_tiles, const float* __restrict__ ee_pose, int cull,
                                                      const float* __restrict__ vis, const int* __restrict__ sel32, const unsigned char* __restrict__ sel8) {
  const int g = blockIdx.x / num, slot = blockIdx.x - g * num;
  if (g >= total_tiles) return;
  if (SEL && !rc_selected(sel32, sel8, slot)) return;
  int k = 0;
  if (n_views > 1 && g >= vt.v[1].tile0) k = 1;
  if (n_views > 2 && g >= vt.v[2].tile0) k = 2;
  if (n_views > 3 && g >= vt.v[3].tile0) k = 3;
  const RpViewEntry& e = vt.v[k];
  rc_draw_tile(m, tab, cnt, e.cam, e.cam_rows, ee_pose, e.width, e.height, cull, e.near_plane, e.far_plane, e.metres, e.rgb, e.depth, e.seg, vis, 0, slot, g - e.tile0,
               e.tiles_x);
}

/* rp_render_points / rp_set_image_points: a fixed-size point cloud per env from the depth (metres) and segmentation layers a draw has just written, one block of four
 * waves per (env, attached view); up to RC_MAX_VIEWS clouds per launch from a by-value table, the view of a block found block-uniformly (blockIdx.x / num).
 *
 * The rule (include/rp_playroom.h; tests/point_cloud_cases.py is its numpy twin): pixels in row-major order i = y width + x; pixel i is VALID iff seg[i] != -1, bit
 * (seg[i] & 0xFF) of drop is clear and (max_depth <= 0 || depth[i] <= max_depth); n = the valid pixels, r(i) = the rank of a valid pixel among them, P = max_points.
 * n <= P: slot r(i) takes pixel i, slots n .. P - 1 are padding (xyz 0, seg -1, rgb 0).  n > P: slot j takes the valid pixel of rank floor(j n / P), 64-bit; those ranks
 * rise strictly with j (n / P > 1), so the thread of rank r decides alone: j0 = ceil(r P / n) is the one slot that can name r, and does iff j0 < P && floor(j0 n / P) == r.
 * count = n, not capped.
 *
 * Two passes over the pixels in chunks of 256, both reading depth / seg coalesced: COUNT (each wave adds up its ballots' popcounts, one LDS word per wave at the end)
 * and PLACE (rank = the running base of the chunks before + the valid pixels of the lower waves of this chunk, from four LDS words per chunk, double-buffered: one
 * barrier per chunk + the lower lanes of the own ballot).  No atomics: the order is the scan order, the same on every run.  The same block then writes the padding and
 * thread 0 the count.  xyz in float32, operation by operation (the build has -ffp-contract=off), in rc_draw_tile's order: nx, ny the pixel's own expressions, z the depth
 * value; RP_POINTS_CAMERA (nx z, ny z, z) along (right, up, forward) - the third component IS the depth value -, RP_POINTS_WORLD eye + ((fwd + right nx) + up ny) z.
 *
 * sel32, sel8: rc_selected by env first + slot; an unselected env's block leaves before it reads or writes anything, ahead of the first barrier.  Every index is
 * bounded where it is made: a pixel by i < width height, a slot by j < P (n <= P: r < n <= P). */
struct RpPointsEntry {
  RpCamera cam; const float* cam_rows;
  int width, height;
  const float* depth; const int* seg; const unsigned char* rgb;                 /* the layers [num][height][width] ([...][3]); rgb only for prgb */
  float* xyz; int* pseg; unsigned char* prgb; int* count;                       /* [num][P][3], [num][P], [num][P][3], [num]; each may be null */
  int max_points, frame; float max_depth; unsigned long long drop;
};
struct RpPointsTable { RpPointsEntry v[RC_MAX_VIEWS]; };

__device__ __forceinline__ bool pc_valid(int sg, float z, float max_depth, unsigned long long drop) {
  const int c = sg & 0xFF;
  return sg != -1 && !(c < 64 && ((drop >> c) & 1ull)) && (max_depth <= 0.f || z <= max_depth);
}

template <bool SEL>
__global__ void __launch_bounds__(256) k_point_cloud(const RpPointsTable pt, int n_views, int num, int first, const float* __restrict__ ee_pose,
                                                     const int* __restrict__ sel32, const unsigned char* __restrict__ sel8) {
  __shared__ float V[14];
  __shared__ int wtot[2][4];
  const int k = blockIdx.x / num, slot = blockIdx.x - k * num;
  if (k >= n_views) return;
  if (SEL && !rc_selected(sel32, sel8, first + slot)) return;
  const RpPointsEntry& e = pt.v[k];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int width = e.width, height = e.height, npix = width * height, P = e.max_points;
  const float max_depth = e.max_depth;
  const unsigned long long drop = e.drop;
  const float* __restrict__ depth = e.depth + (size_t)slot * npix;
  const int* __restrict__ seg = e.seg + (size_t)slot * npix;
  if (tid == 0) rc_view_basis(e.cam, e.cam_rows, ee_pose, slot, V);
  /* COUNT */
  int mine = 0;
  for (int base = 0; base < npix; base += 256) {
    const int i = base + tid;
    const bool ok = i < npix && pc_valid(seg[i], depth[i], max_depth, drop);
    mine += __popcll(__ballot(ok));
  }
  if (lane == 0) wtot[0][wave] = mine;
  __syncthreads();                                       /* (the view is in V from here on, too) */
  const int n = wtot[0][0] + wtot[0][1] + wtot[0][2] + wtot[0][3];
  __syncthreads();
  const V3 eye = ld3(V), fwd = ld3(V + 3), right = ld3(V + 6), up = ld3(V + 9);
  const float thf = V[12], aspect = V[13];
  float* __restrict__ xyz = e.xyz ? e.xyz + (size_t)slot * P * 3 : nullptr;
  int* __restrict__ pseg = e.pseg ? e.pseg + (size_t)slot * P : nullptr;
  unsigned char* __restrict__ prgb = e.prgb ? e.prgb + (size_t)slot * P * 3 : nullptr;
  const unsigned char* __restrict__ rgb = e.rgb ? e.rgb + (size_t)slot * npix * 3 : nullptr;
  /* PLACE */
  int run = 0, buf = 0;
  for (int base = 0; base < npix; base += 256, buf ^= 1) {
    const int i = base + tid;
    int sg = -1; float z = 0.f;
    if (i < npix) { sg = seg[i]; z = depth[i]; }
    const bool ok = i < npix && pc_valid(sg, z, max_depth, drop);
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) wtot[buf][wave] = __popcll(bal);
    __syncthreads();                                     /* one barrier per chunk: the next chunk writes the other buffer, and the one after it comes behind the next barrier */
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const int c = wtot[buf][w]; before += w < wave ? c : 0; all += c; }
    if (ok) {
      const int r = run + before + __popcll(bal & ((1ull << lane) - 1ull));
      long long j = r;
      bool take = true;
      if (n > P) {
        j = ((long long)r * P + n - 1) / n;
        take = j < P && (j * n) / P == r;
      }
      if (take && j < P) {
        if (xyz) {
          const int y = i / width, x = i - y * width;
          const float nx = (2.f * (x + 0.5f) / width - 1.f) * thf * aspect, ny = (1.f - 2.f * (y + 0.5f) / height) * thf;
          float* o = xyz + 3 * (size_t)j;
          if (e.frame == 1) { o[0] = nx * z; o[1] = ny * z; o[2] = z; }
          else {
            o[0] = eye.x + ((fwd.x + right.x * nx) + up.x * ny) * z;
            o[1] = eye.y + ((fwd.y + right.y * nx) + up.y * ny) * z;
            o[2] = eye.z + ((fwd.z + right.z * nx) + up.z * ny) * z;
          }
        }
        if (pseg) pseg[j] = sg;
        if (prgb) { const unsigned char* c = rgb + 3 * (size_t)i; unsigned char* o = prgb + 3 * (size_t)j; o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; }
      }
    }
    run += all;
  }
  for (int j = n + tid; j < P; j += 256) {               /* padding (n < P only) */
    if (xyz) { xyz[3 * (size_t)j] = 0.f; xyz[3 * (size_t)j + 1] = 0.f; xyz[3 * (size_t)j + 2] = 0.f; }
    if (pseg) pseg[j] = -1;
    if (prgb) { prgb[3 * (size_t)j] = 0; prgb[3 * (size_t)j + 1] = 0; prgb[3 * (size_t)j + 2] = 0; }
  }
  if (tid == 0 && e.count) e.count[slot] = n;
}

/* rayTest (environments.py:738-741) for K rays per env: from / to [num][K][3]; fraction 1 and collider -1 on a miss */
__global__ void __launch_bounds__(64) k_ray_test(const DevModel* __restrict__ m, const float* __restrict__ tab, const int* __restrict__ cnt, int num, int K, const float* __restrict__ from,
                                                 const float* __restrict__ to, float* __restrict__ frac, int* __restrict__ collider, int* __restrict__ link,
                                                 float* __restrict__ hit_pos, float* __restrict__ hit_nrm) {
  __shared__ float T[RC_MAX * RC_STRIDE];
  const int slot = blockIdx.x;
  if (slot >= num) return;
  const int n = cnt[slot];
  for (int i = threadIdx.x; i < n * RC_STRIDE; i += 64) T[i] = tab[(size_t)slot * RC_MAX * RC_STRIDE + i];
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 64) {
    const size_t r = (size_t)slot * K + k;
    const V3 o = ld3(from + 3 * r), d = ld3(to + 3 * r) - o;
    float best = 2.f; V3 bn = mk3(0, 0, 0); int bi = -1;
    for (int c = 0; c < n; c++) {
      const float* rec = &T[c * RC_STRIDE];
      if (__float_as_int(rec[18]) & RC_GHOST) continue;
      float t; V3 nn;
      if (rc_hit(m, rec, o, d, 1.f, t, nn) && t < best) { best = t; bn = nn; bi = c; }            /* the lowest collider index wins ties, as in calc_state's ray */
    }
    const bool hit = bi >= 0 && best <= 1.f;
    if (frac) frac[r] = hit ? best : 1.f;
    const int id = hit ? __float_as_int(T[bi * RC_STRIDE + 19]) : -1;
    if (collider) collider[r] = hit ? (id & 0xFF) : -1;
    if (link) link[r] = hit ? (id >> 8) : -1;
    if (hit_pos) st3(hit_pos + 3 * r, hit ? o + d * best : ld3(to + 3 * r));
    if (hit_nrm) st3(hit_nrm + 3 * r, hit ? bn : mk3(0, 0, 0));
  }
}
