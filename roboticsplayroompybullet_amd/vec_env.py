"""VecPlayEnv — N reference environments stepped at once on one MI355X through the C ABI.

Method names, argument meaning and dict keys mirror the reference's playEnv (environments.py:58-314); every value
is a [N, ...] torch tensor on the env's device.  State lives inside the HIP library; the tensors returned by
step()/reset() are owned by this object and overwritten by the next call (clone to keep).
"""
import ctypes as C
import functools
import json
import math
import os

import torch

from . import _lib

OBS_KEYS = ('obs_quat', 'achieved_goal', 'desired_goal', 'controllable_achieved_goal', 'full_positional_state', 'joints',
            'velocity', 'observation')

# record layout of rp_get_state / rp_set_state (csrc/rp_device_model.h ST_*), floats per env = 128
STATE_LAYOUT = {'q': (0, 12), 'qd': (12, 24), 'free0': (24, 37), 'free1': (37, 50), 'jq': (50, 53), 'jqd': (53, 56),
                'motor_mode': (56, 68), 'motor_target': (68, 80), 'motor_maximp': (80, 92), 'goal': (92, 103),
                'last_ee_quat': (103, 107), 'last_block_quat': (107, 111), 'last_ag_quat': (111, 115), 'have_last': (115, 116)}

# the same record in the RP_WIDE build (two-object ids: 9 arm dofs, three free bodies, 18-wide goal)
WIDE_STATE_LAYOUT = {'q': (0, 9), 'qd': (9, 18), 'free0': (18, 31), 'free1': (31, 44), 'free2': (44, 57), 'jq': (57, 60), 'jqd': (60, 63),
                     'motor_mode': (63, 72), 'motor_target': (72, 81), 'motor_maximp': (81, 90), 'goal': (90, 108),
                     'last_ee_quat': (108, 112), 'last_block_quat': (112, 116), 'last_obs_19_23': (116, 120), 'last_ag_10_14': (120, 124),
                     'have_last': (124, 125)}

# registered id -> baked model (the rp_create table: arm + scene)
MODEL_OF = {i: 'URPUUUUUPQQVVVVVVWW'[k] for i, k in _lib.ENV_KINDS.items()}
# scene ids of the complex scene (scenes.py complex_scene, creation order) and of the push scene that the dynamics names call by name; the other
# statics keep their bake tag (static<scene id>)
_SCENE_NAMES = {'complex_scene': {0: 'floor', 1: 'door', 6: 'drawer', 7: 'dial', 8: 'grill', 9: 'button', 10: 'globe', 11: 'table', 12: 'cabinet_back',
                                  13: 'cabinet_top', 14: 'cabinet_left', 15: 'cabinet_right', 16: 'block', 17: 'block2'},
                'push_scene': {0: 'floor', 1: 'tray', 2: 'block'}, 'default_scene': {0: 'floor'}}


@functools.lru_cache(maxsize=None)
def _bake():
    """the models of assets/models.json, read once per process"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'assets', 'models.json')) as f:
        return json.load(f)['models']


def _model(kind):
    return next(m for m in _bake() if m['kind'] == kind)


def _per_model(names):
    """names(model) worked out once per model.  The tuples it holds are shared; a dict of them is handed out as a fresh dict, so callers may change what they get"""
    cached = functools.lru_cache(maxsize=None)(names)

    @functools.wraps(names)
    def fresh(model):
        v = cached(model)
        return dict(v) if isinstance(v, dict) else v
    return fresh


def _check_values(what, v, lo=None, hi=None, problem=None):
    """a host-side value (number, sequence, numpy array, CPU tensor) as a float32 CPU tensor: every entry finite, inside [lo, hi] where given, and problem(t), where
    given, finds nothing to say (it returns the complaint) - ValueError otherwise"""
    t = torch.as_tensor(v, dtype=torch.float32, device='cpu')
    if not bool(torch.isfinite(t).all()):
        raise ValueError('%s: values must be finite' % what)
    if lo is not None and not bool(((t >= lo) & (t <= hi)).all()):
        raise ValueError('%s: values must lie in [%g, %g]' % (what, lo, hi))
    complaint = problem(t) if problem is not None else None
    if complaint:
        raise ValueError(complaint)
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _cam(camera):
    return C.byref(camera) if camera is not None else None


def _depth_mode(depth):
    return _lib.DEPTH_METRES if depth == 'metres' else _lib.DEPTH_BUFFER


@_per_model
def dynamics_names(model):
    """{'friction': names of the collision objects, 'mass': names of the free bodies} of a baked model ('U', 'R', 'P', 'Q', 'V', 'W'), in the column
    order of rp_get_dynamics: objects by their bake number (col_obj), free bodies in the record's order.  Arm links are named by their Bullet link
    index ('link7'), the arm's fixed base 'arm_base', scene bodies as _SCENE_NAMES has them."""
    mdl = _model(model)
    scene = _SCENE_NAMES[mdl['scene']]
    jointed = {j['scene_id'] for j in mdl['joint1']}

    def name(tag, link):
        if tag == 'arm':
            return 'link%d' % link
        if tag.startswith('joint1_'):
            return scene.get(int(tag[7:]), tag)
        if tag.startswith('static') or tag.startswith('free'):
            sid = int(tag.lstrip('staticfre'))
            return scene[sid] + '_base' if sid in jointed and sid in scene else scene.get(sid, tag)      # (the static base of a scene joint's body)
        return tag

    objs = {}
    for c in mdl['col']:
        objs.setdefault(c['obj'], name(c['tag'], c['link']))
    fr = [objs[o] for o in range(len(objs))]
    ms = [scene[b['scene_id']] for b in mdl['free']]
    assert len(set(fr)) == len(fr) and len(set(ms)) == len(ms), (fr, ms)
    return {'friction': tuple(fr), 'mass': tuple(ms)}


def check_dynamics_values(what, v):
    """a host-side friction / mass value (number, sequence, numpy array, CPU tensor) as a float32 CPU tensor; friction must be >= 0, mass > 0, both
    finite (ValueError otherwise)"""
    rule = {'mass': lambda t: None if bool((t > 0).all()) else 'mass: values must be > 0',
            'friction': lambda t: None if bool((t >= 0).all()) else 'friction: values must be >= 0'}
    return _check_values(what, v, problem=rule.get(what))


@_per_model
def wrench_names(model):
    """names of the moving bodies of a baked model, in the column order of rp_get_wrench: the arm's links by their Bullet link index ('link7', one per
    dof, in dof order), the free bodies as dynamics_names' 'mass' calls them ('block', 'drawer', ...), the scene-joint bodies by their scene name
    ('door', 'button', 'dial')"""
    mdl = _model(model)
    scene = _SCENE_NAMES[mdl['scene']]
    names = ['link%d' % a['bullet_index'] for a in mdl['arm']] + list(dynamics_names(model)['mass']) + \
        [scene.get(j['scene_id'], 'joint1_%d' % j['scene_id']) for j in mdl['joint1']]
    assert len(set(names)) == len(names), names
    return tuple(names)


def check_wrench_values(v):
    """a host-side wrench (sequence, numpy array, CPU tensor) as a float32 CPU tensor; every value finite (ValueError otherwise)"""
    return _check_values('wrench', v)


@_per_model
def kinematics_names(model):
    """{'pos': column names of rp_get_kinematics' pos, 'vel': of its vel} of a baked model.  Both start with the arm's dofs as wrench_names names their links
    ('link7', in dof order) and end with the scene joints ('door', 'button', 'dial'); between them every free body of wrench_names has seven pos columns
    ('block.x', '.y', '.z', '.qx', '.qy', '.qz', '.qw') and six vel columns ('block.vx', '.vy', '.vz', '.wx', '.wy', '.wz': world coordinates)"""
    mdl = _model(model)
    names = wrench_names(model)
    na, nf = mdl['n_arm'], len(mdl['free'])
    arm, free, j1 = list(names[:na]), names[na:na + nf], list(names[na + nf:])
    pos = arm + ['%s.%s' % (b, c) for b in free for c in ('x', 'y', 'z', 'qx', 'qy', 'qz', 'qw')] + j1
    vel = arm + ['%s.%s' % (b, c) for b in free for c in ('vx', 'vy', 'vz', 'wx', 'wy', 'wz')] + j1
    assert len(set(pos)) == len(pos) and len(set(vel)) == len(vel), (pos, vel)
    return {'pos': tuple(pos), 'vel': tuple(vel)}


def check_kinematics_values(what, v, names):
    """a host-side pos / vel value (sequence, numpy array, CPU tensor; the last axis runs over `names`, a run of kinematics_names columns) as a float32 CPU
    tensor; every value finite and every quaternion (the four columns from a '.qx' name on) within 1e-3 of unit norm - the library writes the words
    verbatim (ValueError otherwise)"""
    def problem(t):
        if t.dim() == 0 or t.shape[-1] != len(names):
            return '%s: the last axis has %s entries, expected %d' % (what, t.shape[-1] if t.dim() else 'no', len(names))
        for k, nm in enumerate(names):
            if nm.endswith('.qx') and not bool(((t[..., k:k + 4].double().norm(dim=-1) - 1.0).abs() <= 1e-3).all()):
                return '%s: the quaternion %s .. qw must have norm 1 within 1e-3' % (what, nm)

    return _check_values(what, v, problem=problem)


@_per_model
def actuation_names(model):
    """{'gravity': ['x', 'y', 'z'], 'motor': the arm's dofs as wrench_names calls their links ('link7', in dof order)} of a baked model: the columns of
    rp_get_actuation's gravity and of its motor_gain / motor_strength"""
    return {'gravity': ('x', 'y', 'z'), 'motor': tuple('link%d' % a['bullet_index'] for a in _model(model)['arm'])}


ACTUATION_RANGES = {'gravity': (-50.0, 50.0), 'motor_gain': (0.0, 10.0), 'motor_strength': (0.0, 10.0)}


def check_actuation_values(what, v):
    """a host-side gravity / motor_gain / motor_strength value (sequence, numpy array, CPU tensor) as a float32 CPU tensor; finite and inside
    ACTUATION_RANGES (|g| <= 50 per component; 0 <= gain <= 10, which keeps the motor's position gain 0.1 * gain <= 1; 0 <= strength <= 10),
    ValueError otherwise"""
    return _check_values(what, v, *ACTUATION_RANGES[what])


@_per_model
def visual_names(model):
    """a name per collider of a baked model, in collider order (the index ray_test and the segmentation layer report, the rows of get_visuals' colour): the name
    dynamics_names(model)['friction'] gives the collider's collision object, so a name repeats where an object has several colliders (the drawer's five boxes)"""
    objects = dynamics_names(model)['friction']
    return tuple(objects[c['obj']] for c in _model(model)['col'])


@_per_model
def collider_names(model):
    """one UNIQUE name per collider of a baked model, in collider order (the numbers closest_points' pairs, ray_test and the segmentation layer use): visual_names'
    name - the object's, for an arm collider its link's ('link7') - where that names one collider, and name.ordinal ('drawer.0' .. 'drawer.9', in collider order)
    where visual_names repeats it"""
    vis = visual_names(model)
    seen, out = {}, []
    for nm in vis:
        k = seen.get(nm, 0)
        seen[nm] = k + 1
        out.append(nm if vis.count(nm) == 1 else '%s.%d' % (nm, k))
    assert len(set(out)) == len(out), out
    return tuple(out)


VISUAL_WIDTHS = {'colour': 3, 'light': 5, 'background': 3}
LIGHT_DECIMALS = 7      # decimals a host-side light direction is kept to: those of the default direction's literals (csrc/rp_render.cuh VIS_LIGHT_*)


def check_visual_values(what, v):
    """a host-side colour / light / background value (sequence, numpy array, CPU tensor; the last axis is rgb, or for the light dx dy dz ambient diffuse) as a float32
    CPU tensor.  Everything finite; colour and background in [0, 1]; ambient and diffuse >= 0; the light's direction of non-zero length, and normalised here, in float64
    before the float32 cast, because the library uses it as it stands.  The unit vector is kept to seven decimals (LIGHT_DECIMALS), the precision the library's default
    direction is written in (0.2672612, -0.5345225, 0.8017837): (1, -2, 3) gives that row bit for bit, so writing the documented default draws the default image.  A
    component is then within 8e-8 of the float64 unit vector (5e-8 from the decimals, 3e-8 from the cast; the cast alone: 3e-8).  ValueError otherwise."""
    t = torch.as_tensor(v, dtype=torch.float64, device='cpu')
    if t.dim() == 0 or t.shape[-1] != VISUAL_WIDTHS[what]:
        raise ValueError('%s: the last axis has %s entries, expected %d' % (what, t.shape[-1] if t.dim() else 'no', VISUAL_WIDTHS[what]))
    if not bool(torch.isfinite(t).all()):
        raise ValueError('%s: values must be finite' % what)
    if what != 'light':
        return _check_values(what, t, 0.0, 1.0)
    if not bool((t[..., 3:] >= 0).all()):
        raise ValueError('light: ambient and diffuse must be >= 0')
    length = torch.linalg.vector_norm(t[..., :3], dim=-1, keepdim=True)
    if not bool((length > 0).all()):
        raise ValueError('light: the direction must have non-zero length')
    unit = torch.round(t[..., :3] / length * 10.0 ** LIGHT_DECIMALS) / 10.0 ** LIGHT_DECIMALS
    return _check_values(what, torch.cat([unit, t[..., 3:]], dim=-1))


def camera_rows(target=(0.0, 0.25, 0.0), distance=1.3, yaw=-30.0, pitch=-30.0, roll=0.0, fov=50.0, aspect=1.0, n=None):
    """rp_render_layers' cam_rows on the host: a float32 CPU tensor [n, 11] of rows eye[3] target[3] up[3] fov_deg aspect.  Every argument is a scalar or a
    length-n sequence / array / CPU tensor (target: [3] or [n, 3]); n is the longest of them unless given.  Eye and up as rp_camera_from_yaw_pitch_roll computes
    them (float32 arguments, float64 trigonometry, float32 results).  ValueError unless every value is finite, 0 < fov < 180, aspect > 0 and distance > 0."""
    cols = {'distance': distance, 'yaw': yaw, 'pitch': pitch, 'roll': roll, 'fov': fov, 'aspect': aspect}
    cols = {k: _check_values('cameras: ' + k, v).reshape(-1) for k, v in cols.items()}
    tg = _check_values('cameras: target', target)
    if tg.dim() not in (1, 2) or tg.shape[-1] != 3:
        raise ValueError('cameras: target is [3] or [n, 3], not %s' % (tuple(tg.shape),))
    tg = tg.reshape(-1, 3)
    lengths = {int(t.shape[0]) for t in list(cols.values()) + [tg]} - {1}
    if n is None:
        n = max(lengths) if lengths else 1
    if lengths - {int(n)}:
        raise ValueError('cameras: arguments of lengths %s for %d rows' % (sorted(lengths), n))
    cols = {k: t.expand(n) for k, t in cols.items()}
    tg = tg.expand(n, 3)
    if not bool(((cols['fov'] > 0) & (cols['fov'] < 180)).all()):
        raise ValueError('cameras: fov must lie in (0, 180) degrees')
    if not bool((cols['aspect'] > 0).all()) or not bool((cols['distance'] > 0).all()):
        raise ValueError('cameras: aspect and distance must be > 0')
    d2r = 0.01745329251994329547
    y, p, r = (cols[k].double() * d2r for k in ('yaw', 'pitch', 'roll'))
    cy, sy, cp, sp, cr, sr = torch.cos(y), torch.sin(y), torch.cos(p), torch.sin(p), torch.cos(r), torch.sin(r)
    back = torch.stack([cy * sr * sp - sy * cp, sy * sr * sp + cy * cp, cr * sp], 1)      # R's middle column, R = Rz(yaw) Ry(roll) Rx(pitch)
    up = torch.stack([cy * sr * cp + sy * sp, sy * sr * cp - cy * sp, cr * cp], 1)        # ... and its last
    eye = tg + (back * (-cols['distance']).double()[:, None]).float()
    return torch.cat([eye, tg, up.float(), cols['fov'][:, None], cols['aspect'][:, None]], 1).contiguous()


def unpack_segmentation(segmentation):
    """(collider, link) of an rp_render_layers segmentation tensor or array (collider | (link + 1) << 24, -1 on a miss): collider -1 on a miss, link the Bullet
    link index of an arm collider and -1 otherwise - what ray_test reports for the pixel's ray"""
    hit = segmentation >= 0
    return (segmentation & 0xFFFFFF) * hit - (~hit) * 1, (segmentation >> 24) * hit - 1


class VecPlayEnv:
    def __init__(self, env_id, num_envs, device=0, seed=0, env_offset=0, action_type=None, goal_range_low=None, goal_range_high=None,
                 obj_lower_bound=None, obj_upper_bound=None, env_range_high=None, sparse_rew_thresh=None, sparse=True,
                 contact_margin=None, persistent_manifolds=True, hull_gjk=True, speculative_limits=False, hull_epa=None,
                 autoreset=False, max_episode_steps=None, end_on_fault=True, end_on_success=False, reset_table=None):
        """The keyword arguments after env_offset up to hull_epa are the constructor kwargs of the reference's env classes that reach the
        simulation (envList.py -> environments.py:64-67); None keeps what the id registers.  contact_margin: rp_config.

        autoreset=True: step() ends episodes and resets the ended envs on the device (rp_step_autoreset), at the time limit
        (max_episode_steps; None = the id's _max_episode_steps, 0 = none), on a fault (end_on_fault: status & 3), on success
        (end_on_success) and where step's end_mask is set.  reset_table ([M, n_o] tensor, needs autoreset): the ended envs restart from
        its rows with reset(o) semantics instead of a settled reset(), see set_reset_table."""
        if env_id not in _lib.ENV_KINDS:
            raise NotImplementedError('env id %r is outside the hot-path scope (SURVEY.md §8)' % (env_id,))
        if not torch.cuda.is_available():
            raise RuntimeError('VecPlayEnv needs a ROCm GPU: the hot path is HIP-only, there is no CPU fallback')
        self.wide = env_id in _lib.WIDE_IDS
        self.lib = _lib.load(wide=self.wide)
        self.state_layout = WIDE_STATE_LAYOUT if self.wide else STATE_LAYOUT
        self.env_id = env_id
        self.num_envs = int(num_envs)
        idx = device if isinstance(device, int) else (torch.device(device).index or 0)
        self.device = torch.device('cuda', idx)
        # the simulation kwargs (random_start_table builds a handle of the same id with them)
        self._sim_kwargs = dict(action_type=action_type, goal_range_low=goal_range_low, goal_range_high=goal_range_high, obj_lower_bound=obj_lower_bound,
                                obj_upper_bound=obj_upper_bound, env_range_high=env_range_high, sparse_rew_thresh=sparse_rew_thresh, sparse=sparse,
                                contact_margin=contact_margin, persistent_manifolds=persistent_manifolds, hull_gjk=hull_gjk,
                                speculative_limits=speculative_limits, hull_epa=hull_epa)
        cfg = _lib.RpConfig(_lib.ENV_KINDS[env_id], self.num_envs, self.device.index, int(env_offset), int(seed))
        flags = 0
        if (goal_range_low is None) != (goal_range_high is None) or (obj_lower_bound is None) != (obj_upper_bound is None):
            raise ValueError('range kwargs come in low / high pairs')
        if goal_range_low is not None:
            flags |= _lib.CFG_GOAL_RANGE
            cfg.goal_range_low[:] = [float(v) for v in goal_range_low]
            cfg.goal_range_high[:] = [float(v) for v in goal_range_high]
        if obj_lower_bound is not None:
            flags |= _lib.CFG_OBJ_RANGE
            cfg.obj_lower_bound[:] = [float(v) for v in obj_lower_bound]
            cfg.obj_upper_bound[:] = [float(v) for v in obj_upper_bound]
        if env_range_high is not None:
            flags |= _lib.CFG_ENV_RANGE
            cfg.env_range_high[:] = [float(v) for v in env_range_high]
        if sparse_rew_thresh is not None:
            flags |= _lib.CFG_REW_THRESH
            cfg.sparse_rew_thresh = float(sparse_rew_thresh)
        if not sparse:
            flags |= _lib.CFG_DENSE_REWARD
        if action_type is not None:
            flags |= _lib.CFG_ACTION_TYPE
            cfg.action_type = _lib.ACTION_TYPE_CODES[action_type]
        if contact_margin is not None:
            flags |= _lib.CFG_CONTACT_MARGIN
            cfg.contact_margin = float(contact_margin)
        if not persistent_manifolds:
            flags |= _lib.CFG_STATELESS_CONTACTS      # rp_config_flags: no contact cache, points rebuilt every substep (round 3's first model)
        if speculative_limits:
            flags |= _lib.CFG_SPECULATIVE_LIMITS      # round 2's joint-limit rows (oracle rule without bit 2): no gripper chatter, further from Bullet's limit rule
        if not hull_gjk:
            flags |= _lib.CFG_OBB_EDGES               # round 3's contacts where a link's deepest hull vertex lies beside the box face: its OBB instead of GJK on the hull (oracle rule 1015)
        if hull_epa is not None:                      # None: the arm's default (Panda ids: on, UR5 ids: off - include/rp_playroom.h RP_CFG_HULL_EPA)
            flags |= _lib.CFG_HULL_EPA if hull_epa else _lib.CFG_NO_HULL_EPA
        cfg.flags = flags
        self.h = C.c_void_p()
        self._done = None
        self._table_dims = {}      # _dims_of's answers
        self._kept = {}      # entry point -> the tensors its latest call handed to the library: the kernel reads them when the stream gets there
        _lib.check(self.lib, None, self.lib.rp_create(C.byref(cfg), C.byref(self.h)), 'rp_create')
        d = _lib.RpDims()
        self.lib.rp_get_dims(self.h, C.byref(d))
        self.dims = {n: getattr(d, n) for n, _ in _lib.RpDims._fields_}
        N, dev = self.num_envs, self.device

        def f(w):
            return torch.zeros((N, w), dtype=torch.float32, device=dev)

        self.buf = {k: f(self.dims[k]) for k in OBS_KEYS}
        self.buf['gripper_proprioception'] = torch.zeros(N, dtype=torch.int32, device=dev)
        self.buf['reward'] = torch.zeros(N, dtype=torch.float32, device=dev)
        self.buf['is_success'] = torch.zeros(N, dtype=torch.int32, device=dev)
        self.buf['target_poses'] = f(self.dims['target_poses'])
        self.buf['status'] = torch.zeros(N, dtype=torch.int32, device=dev)
        # obs_quat | achieved_goal | reward | is_success in one row per env: the per-step multi-GPU gather's message (sharding.py)
        # (two buffers, alternating per step: an asynchronous gather of step k's pack may still be reading it while step k + 1 runs)
        self._packs = [f(self.dims['obs_quat'] + self.dims['achieved_goal'] + 2) for _ in range(2)]
        self._pack_i = 0
        self.buf['pack'] = self._packs[0]
        self.out = _lib.RpOut(**{k: self.buf[k].data_ptr() for k, _ in _lib.RpOut._fields_})
        at = action_type or _lib.ACTION_TYPES.get(env_id, 'absolute_rpy')                           # environments.py:88-113
        hi = {'absolute_rpy': [6] * 6 + [1], 'absolute_joints': [6] * (self.dims['action'] - 1) + [1]}.get(at, [1] * self.dims['action'])
        self.action_type = at
        self.action_high = torch.tensor(hi, dtype=torch.float32, device=dev)
        self._max_episode_steps = None if env_id.startswith('UR5Play') else 250
        self.record_images = False          # instance.record_images (environments.py:201, 203)
        self.image_envs = None              # (lo, hi): the envs whose img is rendered while record_images is set (default: all - 120 KB per env and call)
        self._img = None                    # reused image buffer: obs['img'] is overwritten by the next step / reset / calc_state (clone() to keep one)
        self.sub_goal = None                # [N, dims.achieved_goal] ghosts drawn into img (visualise_sub_goal)
        self.ghost_arm = None               # [N, 8] ghost arm poses drawn into img (visualise_sub_goal's arm part, Panda ids)
        self.image_obs = None               # set_image_obs: {'rgb' / 'depth' / 'segmentation': the tensors step / reset / calc_state write}, owned like buf
        self.image_final = None             # ... and under autoreset the ended envs' last frames (info['terminal_observation'])
        self.image_cameras = None           # ... and its per-env cameras [N, 11], read on the device at every draw: rewrite rows in place
        self._image_depth = None            # ... and its depth mode ('buffer' / 'metres'; set_image_views: {name: mode}), which set_image_points checks
        self.image_points = None            # set_image_points on set_image_obs' view: {'xyz', 'segmentation', 'count'[, 'rgb']}, obs['points']
        self.image_points_final = None      # ... and under autoreset the ended envs' (info['terminal_observation']['points'])
        self.image_views = None             # set_image_views: {name: {layer: tensor}}, obs['views']; the handle has this configuration or set_image_obs', never both
        self.image_views_final = None       # ... under autoreset {name: {layer: tensor}} of the views with terminal frames (info['terminal_observation']['views'])
        self.image_view_cameras = {}        # ... {name: the per-env cameras [N, 11]} of the views that have them: rewrite rows in place
        self.autoreset = bool(autoreset)
        if self.autoreset:
            limit = self._max_episode_steps if max_episode_steps is None else int(max_episode_steps)
            self.max_episode_steps = limit if limit and limit > 0 else None
            when = _lib.AR_TIME_LIMIT | (_lib.AR_FAULT if end_on_fault else 0) | (_lib.AR_SUCCESS if end_on_success else 0)
            self._call('rp_set_autoreset', self.max_episode_steps or 0, when)
            # the ended envs' step rows (info['terminal_observation']) and the done reasons, owned like buf: overwritten by the next step
            self.final = {k: f(self.dims[k]) for k in OBS_KEYS}
            self.final['gripper_proprioception'] = torch.zeros(N, dtype=torch.int32, device=dev)
            self.final['status'] = torch.zeros(N, dtype=torch.int32, device=dev)
            self.final_out = _lib.RpOut(**{k: self.final[k].data_ptr() for k in self.final})
            self._done_reason = torch.zeros(N, dtype=torch.int32, device=dev)
            self._reset_row = torch.full((N,), -1, dtype=torch.int32, device=dev)      # info['reset_row'], owned like buf
        self._table = None
        if reset_table is not None:
            if not self.autoreset:
                raise ValueError('reset_table needs VecPlayEnv(..., autoreset=True)')
            self.set_reset_table(reset_table)

    def _call(self, fn, *args):
        """self.lib.<fn>(handle, *args); a non-zero return raises RuntimeError with rp_last_error's text"""
        _lib.check(self.lib, self.h, getattr(self.lib, fn)(self.h, *args), fn)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _obs(self):
        o = {k: self.buf[k] for k in OBS_KEYS}
        # environments.py:841-845: img only while record_images is set (render('rgb_array')); all envs, [N, 200, 200, 3] uint8
        o['img'] = None
        if self.image_views is not None:    # set_image_views: the library drew every view inside the call that wrote buf
            o['views'] = self.image_views
            o['img'] = self.image_views.get('img', {}).get('rgb')
        elif self.image_obs is not None:    # set_image_obs: the library drew them inside the call that wrote buf
            o.update(self._image_keys(self.image_obs))
            if self.image_points is not None:
                o['points'] = self.image_points
        elif self.record_images:
            lo, hi = self.image_envs or (0, self.num_envs)
            if self._img is None or self._img.shape[0] != hi - lo:
                self._img = torch.empty((hi - lo, 200, 200, 3), dtype=torch.uint8, device=self.device)
            sg = self.sub_goal[lo:hi] if (self.sub_goal is not None and self.sub_goal.shape[0] == self.num_envs) else self.sub_goal
            ga = self.ghost_arm[lo:hi] if (self.ghost_arm is not None and self.ghost_arm.shape[0] == self.num_envs) else self.ghost_arm
            o['img'] = self.render('rgb_array', envs=(lo, hi), sub_goal=sg, out=self._img, ghost_arm=ga)
        o['gripper_proprioception'] = self.buf['gripper_proprioception']
        return o

    def close(self):
        if getattr(self, 'h', None):
            self.lib.rp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _flip_pack(self, keep_rows=False):
        """the next writer of the pack gets the other buffer: an asynchronous gather of the previous step's pack (sharding.gather_observations,
        on RCCL's stream) may still be reading the current one, and nothing orders a write on our stream after that read.  keep_rows: a masked
        reset rewrites only some rows, so the others are carried over first (a device copy on our stream that only READS the old buffer)."""
        new = self._packs[self._pack_i ^ 1]
        if keep_rows:
            new.copy_(self._packs[self._pack_i])
        self._pack_i ^= 1
        self.buf['pack'] = new
        self.out.pack = new.data_ptr()

    def reset(self, mask=None, o=None):
        """playEnv.reset(o=None) for all envs (or those where mask != 0).  With o [N, >= 18 / 10 / 3]: playEnv.reset(o) - objects
        and arm are placed from the observation vectors instead of being sampled (environments.py:542-556, 575-590)."""
        mp = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mp = _ptr(mask)
        self._flip_pack(keep_rows=mask is not None)
        if o is None:
            self._call('rp_reset', mp, C.byref(self.out), self._stream())
        else:
            o = o.to(device=self.device, dtype=torch.float32).contiguous()
            assert o.dim() == 2 and o.shape[0] == self.num_envs, o.shape
            self._call('rp_reset_to', _ptr(o), o.shape[1], mp, C.byref(self.out), self._stream())
        return self._obs()

    def step(self, action, end_mask=None):
        """playEnv.step for every env.  With autoreset: the envs whose episode ended (time limit, fault, success, end_mask [N] != 0) are
        reset inside the call, on the device - obs holds their new episode's first observation, the reward / is_success the transition's;
        done is a bool [N] tensor, info['terminal_observation'] the ended envs' step observations (rows valid where done),
        info['done_reason'] the int32 reasons (_lib.DONE_*), info['TimeLimit.truncated'] the envs that the time limit alone ended.  After
        set_image_obs the obs and, with autoreset, info['terminal_observation'] carry the camera images drawn inside the same call."""
        a = action.to(device=self.device, dtype=torch.float32).contiguous()
        assert a.shape == (self.num_envs, self.dims['action']), a.shape
        if self.autoreset:
            return self._step_autoreset(a, end_mask)
        assert end_mask is None, 'end_mask needs VecPlayEnv(..., autoreset=True)'
        self._flip_pack()
        self._call('rp_step', _ptr(a), C.byref(self.out), self._stream())
        info = {'is_success': self.buf['is_success'], 'target_poses': self.buf['target_poses'], 'status': self.buf['status']}
        if self._done is None:      # environments.py:212: always False - one tensor for the handle's life (a fill kernel per step sat at the end of the step's chain: 8 us)
            self._done = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        return self._obs(), self.buf['reward'], self._done, info

    def _step_autoreset(self, a, end_mask):
        mp = None
        if end_mask is not None:
            end_mask = end_mask.to(device=self.device, dtype=torch.uint8).contiguous()
            assert end_mask.shape == (self.num_envs,), end_mask.shape
            mp = _ptr(end_mask)
        self._flip_pack()
        self._call('rp_step_autoreset', _ptr(a), mp, C.byref(self.out), C.byref(self.final_out), _ptr(self._done_reason), self._stream())
        if self._table is not None:
            self._call('rp_get_reset_rows', _ptr(self._reset_row), self._stream())
        reason = self._done_reason
        info = {'is_success': self.buf['is_success'], 'target_poses': self.buf['target_poses'], 'status': self.buf['status'],
                'terminal_observation': {k: self.final[k] for k in OBS_KEYS + ('gripper_proprioception',)},
                'terminal_status': self.final['status'],
                'TimeLimit.truncated': reason == _lib.DONE_TIME_LIMIT,      # gym 0.21: the time limit and nothing else ended the episode
                'done_reason': reason,
                'reset_row': self._reset_row}      # the table row each ended env restarted from, -1 elsewhere (and everywhere without a table)
        if self.image_final is not None:
            info['terminal_observation'].update(self._image_keys(self.image_final))
            if self.image_points_final is not None:
                info['terminal_observation']['points'] = self.image_points_final
        if self.image_views_final is not None:
            info['terminal_observation']['views'] = self.image_views_final
        return self._obs(), self.buf['reward'], reason != 0, info

    def set_reset_table(self, o):
        """o [M, n_o]: the ended envs of the following autoreset steps restart from its rows with reset(o) semantics (rp_reset_to) - the ended env
        of rank k in a step (counting ended envs in env order) takes row (cursor + k) mod M, and the cursor, 0 after this call, moves on by the step's
        ends.  A row of obs_quat of the same id is a valid o, except on the two-object ids: reset(o) reads 28 entries there, obs_quat has 26.  None
        removes the table: ended envs get a settled reset() again.  Synchronises the device (the table it replaces may still be read by steps in
        flight)."""
        if not self.autoreset:
            raise ValueError('set_reset_table needs VecPlayEnv(..., autoreset=True)')
        if o is None:
            self._call('rp_set_reset_table', None, 0, 0, self._stream())
            self._table = None
            self._reset_row.fill_(-1)
            return
        o = torch.as_tensor(o).to(device=self.device, dtype=torch.float32).contiguous()
        assert o.dim() == 2 and o.shape[0] > 0, o.shape
        self._call('rp_set_reset_table', _ptr(o), o.shape[0], o.shape[1], self._stream())
        self._table = o      # (kept until the next set: the copy reads it when the stream gets there)

    def random_start_table(self, m, seed):
        """[m, obs_quat] float32: the obs_quat rows of m fresh reset()s (a temporary handle of this id and simulation kwargs, seed `seed`,
        env_offset 0) - a table for set_reset_table that gives near-random starts without the settle.  reset(o) from such a row is not the
        reset() it came from: the objects are placed at the observed poses (the play ids; the others at the observed positions, unrotated) with
        zero velocities, where the settled ones may still have been moving; the arm is solved by IK from the rest pose toward the observed
        end-effector position and, on the play ids, orientation - reset() aimed it at a random target with the default orientation; and the goal
        is drawn anew (again while it is already solved).  On the play ids, reset(o) reads the blocks from o[11 + 10 b : 18 + 10 b] as the
        reference does, which in an obs_quat row is not the block's pose; and on the two-object ids the rows are
        shorter than what reset(o) reads (26 < 28), so set_reset_table refuses them unwidened."""
        tmp = VecPlayEnv(self.env_id, int(m), device=self.device.index, seed=seed, **self._sim_kwargs)
        try:
            return tmp.reset()['obs_quat'].clone()
        finally:
            torch.cuda.synchronize(self.device)
            tmp.close()

    @property
    def episode_steps(self):
        """int32 [N]: steps of every env's current episode (rp_step_autoreset counts them; reset() sets the reset envs' to 0)"""
        t = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._call('rp_get_episode_steps', _ptr(t), self._stream())
        return t

    @episode_steps.setter
    def episode_steps(self, steps):
        """e.g. env.episode_steps = torch.arange(N) % limit: staggered time limits"""
        t = torch.as_tensor(steps).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        assert t.shape == (self.num_envs,), t.shape
        self._call('rp_set_episode_steps', _ptr(t), self._stream())
        self._kept['rp_set_episode_steps'] = t      # (kept until the next set: the copy reads it when the stream gets there)

    # ---- the per-env parameter tables and the state by column: every setter is _block per argument, _same_rows, _mask, one _call
    def _dims_of(self, fn, n):
        """the n int32 results of an rp_get_*_dims call: constants of the handle, so the library is asked once"""
        dims = self._table_dims.get(fn)
        if dims is None:
            d = [C.c_int32() for _ in range(n)]
            self._call(fn, *[C.byref(x) for x in d])
            dims = self._table_dims[fn] = [x.value for x in d]
        return dims

    def _empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _block(self, fn, what, v, shape, check, scalar=False):
        """The argument `what` of `fn`, a value for a block of `shape` ((k,); (n_body, 6) for the wrench table; () for one joint) or for N of them, as (contiguous
        float32 device tensor, rows = 1 or N); None gives (None, 0).  A tensor on the env's device goes through without a host read; any other value goes through
        check (a check_*_values) and then to the device.  scalar: a host number stands for the whole block.  Another shape is a ValueError."""
        if v is None:
            return None, 0
        N = self.num_envs
        on_dev = isinstance(v, torch.Tensor) and v.device == self.device
        t = v.to(dtype=torch.float32) if on_dev else check(v).to(self.device)
        if scalar and t.dim() == 0 and not on_dev:
            t = t.expand(shape)
        got = tuple(t.shape)
        if got == shape:
            return t.contiguous(), 1
        if got == (N,) + shape:
            return t.contiguous(), N

        def text(sh):
            return '[%s]' % ', '.join('%d' % n for n in sh)
        raise ValueError('%s: %s has shape %s, expected %s or %s' % (fn, what, got, text(shape) if shape else 'a number', text((N,) + shape)))

    def _same_rows(self, parts):
        """the (tensor or None, rows) of one call's arguments -> ([tensor or None], rows): one call, one row count, so single rows are expanded to N when another
        argument has N"""
        rows = max(r for _, r in parts)
        return [t.expand(self.num_envs, *t.shape).contiguous() if t is not None and r != rows else t for t, r in parts], rows

    def _mask(self, what, mask):
        if mask is None:
            return None
        mask = mask.to(device=self.device, dtype=torch.uint8).contiguous() if isinstance(mask, torch.Tensor) else \
            torch.as_tensor(mask, dtype=torch.uint8).to(self.device)
        if mask.shape != (self.num_envs,):
            raise ValueError('%s: mask has shape %s, expected [%d]' % (what, tuple(mask.shape), self.num_envs))
        return mask

    @property
    def dynamics_names(self):
        """{'friction': a name per collision object, 'mass': a name per free body}: the columns of get_dynamics / set_dynamics"""
        return dynamics_names(MODEL_OF[self.env_id])

    def get_dynamics(self):
        """{'friction': [N, n_obj], 'mass': [N, n_free]} float32 device tensors: every env's lateral friction per collision object and mass per
        free body (a fresh handle: the baked values)"""
        no, nf = self._dims_of('rp_get_dynamics_dims', 2)
        fr, ms = self._empty(self.num_envs, no), self._empty(self.num_envs, nf)
        self._call('rp_get_dynamics', _ptr(fr), _ptr(ms) if nf else None, self._stream())
        return {'friction': fr, 'mass': ms}

    def set_dynamics(self, friction=None, mass=None, mask=None):
        """Per-env lateral friction per collision object ([N, n_obj] or [n_obj]: every env the same) and / or mass per free body ([N, n_free] or
        [n_free]) for the envs where mask [N] != 0 (None: all); None leaves that parameter as it is.  A contact's friction is the product of its
        objects' (at most 10); a body's inertia scales with its mass.  The values act from the next step or reset substep on this stream, and no
        reset changes them.  Host values (numbers, numpy, CPU tensors) are checked (friction >= 0, mass > 0, finite); tensors on the env's device
        are passed through without a host read, so the call can sit in a device-side loop (e.g. mask=done)."""
        if friction is None and mass is None:
            raise ValueError('set_dynamics: give friction, mass or both')
        widths = self._dims_of('rp_get_dynamics_dims', 2)
        (fr, ms), rows = self._same_rows([self._block('set_dynamics', what, v, (k,), lambda x, what=what: check_dynamics_values(what, x), scalar=True)
                                          for what, v, k in zip(('friction', 'mass'), (friction, mass), widths)])
        mask = self._mask('set_dynamics', mask)
        self._call('rp_set_dynamics', _ptr(fr), _ptr(ms) if ms is not None and ms.numel() else None, rows, _ptr(mask), self._stream())
        self._kept['rp_set_dynamics'] = (fr, ms, mask)      # (kept until the next set: the kernel reads them when the stream gets there)

    @property
    def wrench_names(self):
        """a name per moving body: the body columns of get_wrench / set_wrench (arm links, free bodies, scene-joint bodies)"""
        return wrench_names(MODEL_OF[self.env_id])

    def _n_body(self):
        return sum(self._dims_of('rp_get_wrench_dims', 3))

    def get_wrench(self):
        """[N, n_body, 6] float32 device tensor: every env's external force (through the centre of mass) and torque on each moving body, world
        coordinates, fx fy fz tx ty tz (a fresh handle: zeros)"""
        w = self._empty(self.num_envs, self._n_body(), 6)
        self._call('rp_get_wrench', _ptr(w), self._stream())
        return w

    def set_wrench(self, wrench, mask=None):
        """External wrenches ([N, n_body, 6], or [n_body, 6]: every env the same; None: zero) for the envs where mask [N] != 0 (None: all).  Bodies as
        wrench_names has them; per body a world force through its centre of mass and a world torque.  They act in every substep from the next step or
        reset substep on this stream until they are set again; no reset changes them.  Host values (sequences, numpy, CPU tensors) are checked finite;
        tensors on the env's device are passed through without a host read, so the call can sit in a device-side loop (set_wrench(None, mask=done))."""
        w, rows = self._block('set_wrench', 'wrench', wrench, (self._n_body(), 6), check_wrench_values)
        mask = self._mask('set_wrench', mask)
        self._call('rp_set_wrench', _ptr(w), rows or 1, _ptr(mask), self._stream())
        self._kept['rp_set_wrench'] = (w, mask)      # (kept until the next set: the kernel reads them when the stream gets there)

    def push(self, body, force=None, torque=None, mask=None):
        """Set the force and / or the torque (3 values, or [N, 3]; None leaves that half as it is) on one body of wrench_names for the envs where
        mask != 0 (None: all), the other bodies' wrenches untouched: a read-modify-write of the table on the device."""
        if force is None and torque is None:
            raise ValueError('push: give force, torque or both')
        b = self.wrench_names.index(body)
        w = self.get_wrench()
        for half, what, v in ((0, 'force', force), (1, 'torque', torque)):
            if v is not None:
                w[:, b, 3 * half:3 * half + 3] = self._block('push', what, v, (3,), check_wrench_values)[0]
        self.set_wrench(w, mask=mask)

    @property
    def actuation_names(self):
        """{'gravity': ('x', 'y', 'z'), 'motor': a name per arm dof}: the columns of get_actuation / set_actuation"""
        return actuation_names(MODEL_OF[self.env_id])

    def _n_arm(self):
        return self._dims_of('rp_get_actuation_dims', 1)[0]

    def get_actuation(self):
        """{'gravity': [N, 3], 'motor_gain': [N, n_arm], 'motor_strength': [N, n_arm]} float32 device tensors: every env's gravity vector (m/s^2,
        world) and the gain and strength factor of each arm motor in dof order (a fresh handle: (0, 0, -9.8), ones, ones)"""
        N, na = self.num_envs, self._n_arm()
        g, kp, st = self._empty(N, 3), self._empty(N, na), self._empty(N, na)
        self._call('rp_get_actuation', _ptr(g), _ptr(kp), _ptr(st), self._stream())
        return {'gravity': g, 'motor_gain': kp, 'motor_strength': st}

    def set_actuation(self, gravity=None, motor_gain=None, motor_strength=None, mask=None):
        """Per-env gravity vector ([N, 3] or [3]: every env the same) and / or a gain and a strength factor per arm motor ([N, n_arm] or [n_arm], dof
        order: actuation_names['motor']) for the envs where mask [N] != 0 (None: all); None leaves that parameter as it is.  Gravity acts on the arm,
        the free bodies and the prismatic scene joints; an arm motor asks for 0.1 * gain * (target - q) / dt and is bounded by strength times the
        impulse the action gave it (strength 0: the motor is off).  The values act from the next step or reset substep on this stream, and no reset
        changes them.  Host values (sequences, numpy, CPU tensors) are checked (|g| <= 50 per component, 0 <= gain <= 10, 0 <= strength <= 10,
        finite); tensors on the env's device are passed through without a host read, so the call can sit in a device-side loop (e.g. mask=done)."""
        if gravity is None and motor_gain is None and motor_strength is None:
            raise ValueError('set_actuation: give gravity, motor_gain, motor_strength or several')
        na = self._n_arm()
        parts, rows = self._same_rows([self._block('set_actuation', what, v, (k,), lambda x, what=what: check_actuation_values(what, x))
                                       for what, v, k in (('gravity', gravity, 3), ('motor_gain', motor_gain, na), ('motor_strength', motor_strength, na))])
        mask = self._mask('set_actuation', mask)
        self._call('rp_set_actuation', *[_ptr(t) for t in parts], rows, _ptr(mask), self._stream())
        self._kept['rp_set_actuation'] = (parts, mask)      # (kept until the next set: the kernel reads them when the stream gets there)

    @property
    def visual_names(self):
        """a name per collider, in collider order: the rows of get_visuals' colour (the collider's object as dynamics_names['friction'] calls it; names repeat)"""
        return visual_names(MODEL_OF[self.env_id])

    def _n_col(self):
        return self._dims_of('rp_get_visuals_dims', 1)[0]

    def get_visuals(self):
        """{'colour': [N, n_col, 3], 'light': [N, 5], 'background': [N, 3]} float32 device tensors: every env's rgb per collider (collider order: visual_names), its
        light (direction towards it dx dy dz, ambient, diffuse) and the colour of a miss (a fresh handle: the reference's colours, (1, -2, 3) / sqrt(14) with 0.45
        and 0.55, and (0.82, 0.88, 0.96)).  The first get_visuals or set_visuals of a handle allocates the table (up to 800 bytes per env)."""
        N, nc = self.num_envs, self._n_col()
        col, light, bg = self._empty(N, nc, 3), self._empty(N, 5), self._empty(N, 3)
        self._call('rp_get_visuals', _ptr(col), _ptr(light), _ptr(bg), self._stream())
        return {'colour': col, 'light': light, 'background': bg}

    def set_visuals(self, colour=None, light=None, background=None, mask=None):
        """Per-env appearance of the camera images: colour per collider ([N, n_col, 3] or [n_col, 3]: every env the same; rgb in 0 .. 1, collider order:
        visual_names), light ([N, 5] or [5]: direction towards the light, ambient, diffuse - a hit is drawn as colour * (ambient + diffuse * max(0, n . direction)))
        and background ([N, 3] or [3]: the colour of a miss) for the envs where mask [N] != 0 (None: all); None leaves that part as it is.  render, render_layers'
        rgb and - since it goes through render - obs['img'] under record_images draw with them from the next call on this stream, ghosts included; depth,
        segmentation and ray_test do not read them, and the button's globe and the dial's grill keep showing their state in red / white.  No reset, set_state or
        clone_envs changes them.  Host values (sequences, numpy, CPU tensors) are checked (finite, colours in [0, 1], ambient and diffuse >= 0) and the light's
        direction is normalised (check_visual_values: (1, -2, 3) is the default direction bit for bit); tensors on the env's device are passed through without a host read and used as they stand, so the call can sit in a device-side
        loop (e.g. mask=done)."""
        if colour is None and light is None and background is None:
            raise ValueError('set_visuals: give colour, light, background or several')
        parts, rows = self._same_rows([self._block('set_visuals', what, v, shape, lambda x, what=what: check_visual_values(what, x))
                                       for what, v, shape in (('colour', colour, (self._n_col(), 3)), ('light', light, (5,)), ('background', background, (3,)))])
        mask = self._mask('set_visuals', mask)
        self._call('rp_set_visuals', *[_ptr(t) for t in parts], rows, _ptr(mask), self._stream())
        self._kept['rp_set_visuals'] = (parts, mask)      # (kept until the next set: the kernel reads them when the stream gets there)

    def set_colour(self, name, rgb, mask=None):
        """Set the colour (3 values, or [N, 3]) of every collider of one object of visual_names for the envs where mask != 0 (None: all), the other colliders'
        colours untouched: a read-modify-write of the colour table on the device.  An unknown name is a KeyError that lists the names."""
        names = self.visual_names
        cols = [c for c, nm in enumerate(names) if nm == name]
        if not cols:
            raise KeyError('set_colour: no object %r; the names are %s' % (name, ', '.join(sorted(set(names)))))
        colour = self.get_visuals()['colour']
        v = self._block('set_colour', 'rgb', rgb, (3,), lambda x: check_visual_values('colour', x))[0]
        colour[:, cols, :] = v.reshape(-1, 1, 3)
        self.set_visuals(colour=colour, mask=mask)

    @property
    def kinematics_names(self):
        """{'pos': a name per column of get_kinematics()['pos'], 'vel': of ['vel']}: arm dofs, free bodies' pose / velocity components, scene joints"""
        return kinematics_names(MODEL_OF[self.env_id])

    def get_kinematics(self):
        """{'pos': [N, n_pos], 'vel': [N, n_vel]} float32 device tensors: every env's joint positions, free-body poses (x y z qx qy qz qw) and scene-joint
        positions, and the matching velocities (free bodies: world linear and angular), columns as kinematics_names has them"""
        names = self.kinematics_names
        p, v = self._empty(self.num_envs, len(names['pos'])), self._empty(self.num_envs, len(names['vel']))
        self._call('rp_get_kinematics', _ptr(p), _ptr(v), self._stream())
        return {'pos': p, 'vel': v}

    def set_kinematics(self, pos=None, vel=None, mask=None, clear_contacts=False):
        """Write joint positions / body poses ([N, n_pos] or [n_pos]: every env the same) and / or velocities ([N, n_vel] or [n_vel]) into the state of the envs
        where mask [N] != 0 (None: all); None leaves that half as it is.  The words are written verbatim and nothing else changes (motor targets, goal,
        quaternion memory, RNG and episode counters, parameter tables); the contact cache stays unless clear_contacts, which gives the masked envs a state
        without contact history.  Host values (sequences, numpy, CPU tensors) are checked (finite, unit quaternions within 1e-3); tensors on the env's device
        are passed through without a host read, so the call can sit in a device-side loop (e.g. mask=done)."""
        if pos is None and vel is None:
            raise ValueError('set_kinematics: give pos, vel or both')
        names = self.kinematics_names
        parts, rows = self._same_rows([self._block('set_kinematics', what, v, (len(names[what]),), lambda x, what=what: check_kinematics_values(what, x, names[what]))
                                       for what, v in (('pos', pos), ('vel', vel))])
        mask = self._mask('set_kinematics', mask)
        self._call('rp_set_kinematics', *[_ptr(t) for t in parts], rows, _ptr(mask), _lib.KIN_CLEAR_CONTACTS if clear_contacts else 0, self._stream())
        self._kept['rp_set_kinematics'] = (parts, mask)      # (kept until the next set: the kernel reads them when the stream gets there)

    def set_body(self, name, pos=None, quat=None, lin_vel=None, ang_vel=None, mask=None, clear_contacts=False):
        """Place one free body of wrench_names ('block', 'drawer', ...): position (3 values or [N, 3]), orientation quaternion (xyzw, 4 or [N, 4]), world linear
        and angular velocity (3 or [N, 3]) for the envs where mask != 0 (None: all); None leaves that part as it is.  A read of the tables, a column
        assignment on the device and set_kinematics; an unknown name raises KeyError."""
        if pos is None and quat is None and lin_vel is None and ang_vel is None:
            raise ValueError('set_body: give pos, quat, lin_vel, ang_vel or several')
        names = self.kinematics_names
        if name + '.x' not in names['pos']:
            raise KeyError('set_body: %r is not a free body of %s' % (name, self.env_id))
        p0, v0 = names['pos'].index(name + '.x'), names['vel'].index(name + '.vx')
        kin = self.get_kinematics()
        for what, tab, v, c0, k in (('pos', 'pos', pos, p0, 3), ('quat', 'pos', quat, p0 + 3, 4), ('lin_vel', 'vel', lin_vel, v0, 3), ('ang_vel', 'vel', ang_vel, v0 + 3, 3)):
            if v is not None:
                cols = names[tab][c0:c0 + k]
                kin[tab][:, c0:c0 + k] = self._block('set_body', what, v, (k,), lambda x: check_kinematics_values('set_body: ' + what, x, cols))[0]
        self.set_kinematics(pos=kin['pos'] if pos is not None or quat is not None else None,
                            vel=kin['vel'] if lin_vel is not None or ang_vel is not None else None, mask=mask, clear_contacts=clear_contacts)

    def set_joint(self, name, q=None, qd=None, mask=None):
        """Set the position and / or velocity (a number or [N]) of one arm dof ('link7') or scene joint ('door', 'button', 'dial') for the envs where mask != 0
        (None: all); None leaves that half as it is.  The arm's motors keep their targets: a position-controlled dof is driven back unless the next action
        asks for the new position.  An unknown name raises KeyError."""
        if q is None and qd is None:
            raise ValueError('set_joint: give q, qd or both')
        names = self.kinematics_names
        if name not in names['pos'] or '.' in name:
            raise KeyError('set_joint: %r is neither a dof nor a scene joint of %s' % (name, self.env_id))
        kin = self.get_kinematics()

        def number(what, x):      # (this call looks at a host value's shape before its entries: a wrongly shaped one goes to _block unchecked, which refuses it)
            t = torch.as_tensor(x, dtype=torch.float32, device='cpu')
            return _check_values('set_joint: ' + what, t) if tuple(t.shape) in ((), (self.num_envs,)) else t

        for what, tab, v in (('q', 'pos', q), ('qd', 'vel', qd)):
            if v is not None:
                kin[tab][:, names[tab].index(name)] = self._block('set_joint', what, v, (), functools.partial(number, what))[0]
        self.set_kinematics(pos=kin['pos'] if q is not None else None, vel=kin['vel'] if qd is not None else None, mask=mask)

    def clone_envs(self, src, mask=None, episode_steps=True):
        """Every env e where mask [N] != 0 (None: all) becomes a copy of env src[e] as it was before the call (src: int tensor or sequence [N]): state record
        and contact cache, and with episode_steps its episode counter - on the device, for any src (permutations, many-to-one: resampling, broadcasting one
        env to a population).  The parameter tables (dynamics, wrench, actuation) and the reset table are not copied.  A host src is range-checked
        (ValueError); a tensor on the env's device is passed through without a host read, and an entry outside [0, N) leaves its env unchanged."""
        N = self.num_envs
        if isinstance(src, torch.Tensor) and src.device == self.device:
            if src.dtype.is_floating_point or src.dtype == torch.bool:
                raise ValueError('clone_envs: src must be an integer tensor')
            t = src.to(dtype=torch.int32)
        else:
            t = torch.as_tensor(src, device='cpu')
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise ValueError('clone_envs: src must hold integers')
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= N):
                raise ValueError('clone_envs: src must lie in [0, %d)' % N)
            t = t.to(dtype=torch.int32).to(self.device)
        if t.shape != (N,):
            raise ValueError('clone_envs: src has shape %s, expected [%d]' % (tuple(t.shape), N))
        t = t.contiguous()
        mask = self._mask('clone_envs', mask)
        self._call('rp_copy_envs', _ptr(t), _ptr(mask), _lib.COPY_EPISODE_STEPS if episode_steps else 0, self._stream())
        self._kept['rp_copy_envs'] = (t, mask)      # (kept until the next call: the kernel reads them when the stream gets there)

    def calc_state(self):
        self._flip_pack()
        self._call('rp_calc_state', C.byref(self.out), self._stream())
        return self._obs()

    def reset_goal_pos(self, goal=None, mask=None):
        gp = mp = None
        if goal is not None:
            goal = goal.to(device=self.device, dtype=torch.float32).contiguous()
            assert goal.shape == (self.num_envs, self.dims['desired_goal'])
            gp = _ptr(goal)
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mp = _ptr(mask)
        self._call('rp_reset_goal', gp, mp, self._stream())

    def compute_reward_sparse(self, achieved_goal, desired_goal, info=None):
        """the sparse formula (environments.py:278-304) whatever `sparse` the env was built with"""
        return self.compute_reward(achieved_goal, desired_goal, info, _fn='rp_compute_reward_sparse')

    def compute_reward(self, achieved_goal, desired_goal, info=None, _fn='rp_compute_reward'):
        ag = achieved_goal.to(device=self.device, dtype=torch.float32).contiguous()
        dg = desired_goal.to(device=self.device, dtype=torch.float32).contiguous()
        w = self.dims['achieved_goal']
        ag2, dg2 = ag.reshape(-1, w), dg.reshape(-1, w)
        r = torch.empty(ag2.shape[0], dtype=torch.float32, device=self.device)
        self._call(_fn, _ptr(ag2), _ptr(dg2), _ptr(r), ag2.shape[0], self._stream())
        return r.reshape(ag.shape[:-1])

    @property
    def pack(self):
        """[N, obs_quat + achieved_goal + 2] written by the latest step / reset / calc_state: obs_quat | achieved_goal | reward |
        is_success (float)"""
        return self.buf['pack']

    def camera(self, target=(0.0, 0.25, 0.0), distance=1.3, yaw=-30.0, pitch=-30.0, roll=0.0, fov=50.0, aspect=1.0, gripper=False):
        """an rp_camera: p.computeViewMatrixFromYawPitchRoll + computeProjectionMatrixFOV (the defaults are the reference's fixed camera,
        environments.py:21-30); gripper=True: the gripper camera of environments.py:33-49"""
        cam = _lib.RpCamera()
        _lib.check(self.lib, self.h, self.lib.rp_camera_from_yaw_pitch_roll((C.c_float * 3)(*[float(v) for v in target]), float(distance), float(yaw),
                                                                             float(pitch), float(roll), C.byref(cam)), 'rp_camera_from_yaw_pitch_roll')
        cam.fov_deg, cam.aspect, cam.mode = float(fov), float(aspect), 1 if gripper else 0
        return cam

    def render(self, mode='rgb_array', width=200, height=200, envs=None, camera=None, sub_goal=None, out=None, ghost_arm=None):
        """obs['img'] of the reference (environments.py:841-845: getCameraImage(200, 200, ...)[2][:, :, :3]) for envs [lo, hi) (default: all):
        uint8 [n, height, width, 3] on the device.  sub_goal [n, dims.achieved_goal]: draw the sub-goal's ghosts
        (visualise_sub_goal, environments.py:606-690).  ghost_arm [n, 8] = EE position, orientation quaternion (xyzw), gripper: the ghost ARM of
        visualise_sub_goal's 'controllable_achieved_goal' / 'full_positional_state' (environments.py:623-637, 671-674; Panda ids only - the reference raises for the
        UR5).  mode 'human' (a GUI window) does not exist here and returns None."""
        if mode == 'human':
            return None
        lo, n, sub_goal, ghost_arm = self._render_args(envs, sub_goal, ghost_arm)
        img = out if out is not None else torch.empty((n, int(height), int(width), 3), dtype=torch.uint8, device=self.device)
        assert img.shape == (n, int(height), int(width), 3) and img.dtype == torch.uint8 and img.is_contiguous()
        head = (_cam(camera), int(width), int(height), lo, n, _ptr(img), _ptr(sub_goal))
        if ghost_arm is not None:
            self._call('rp_render_ex', *head, _ptr(ghost_arm), self._stream())
        else:
            self._call('rp_render', *head, self._stream())
        return img

    def _render_args(self, envs, sub_goal, ghost_arm):
        """render's and render_layers': (first env, number of envs, sub_goal, ghost_arm), the two float32, contiguous, on the device and of one row per env (or None)"""
        lo, hi = (0, self.num_envs) if envs is None else (int(envs[0]), int(envs[1]))
        n = hi - lo
        if sub_goal is not None:
            sub_goal = sub_goal.to(device=self.device, dtype=torch.float32).contiguous()
            assert sub_goal.shape == (n, self.dims['achieved_goal']), sub_goal.shape
        if ghost_arm is not None:
            ghost_arm = ghost_arm.to(device=self.device, dtype=torch.float32).contiguous()
            assert ghost_arm.shape == (n, 8), ghost_arm.shape
        return lo, n, sub_goal, ghost_arm

    def cameras(self, target=(0.0, 0.25, 0.0), distance=1.3, yaw=-30.0, pitch=-30.0, roll=0.0, fov=50.0, aspect=1.0):
        """per-env cameras for render_layers(cameras=...): the float32 device tensor [n, 11] of camera_rows (each argument a scalar or a length-n host array or
        tensor; all scalars: n = num_envs).  Host values are range-checked (ValueError): 0 < fov < 180, aspect > 0, distance > 0.  A tensor of the same layout built
        on the device goes to render_layers as it is, unchecked and unread."""
        scalars = all(torch.as_tensor(v).dim() == 0 for v in (distance, yaw, pitch, roll, fov, aspect)) and torch.as_tensor(target).dim() == 1
        return camera_rows(target, distance, yaw, pitch, roll, fov, aspect, n=self.num_envs if scalars else None).to(self.device)

    unpack_segmentation = staticmethod(unpack_segmentation)

    def _layer_args(self, who, n, width, height, layers, depth, camera, cameras, near, far):
        """render_layers' and set_image_obs' host-side checks (ValueError): (the layers as a tuple, {layer: (shape, dtype)} for n envs, cameras contiguous or None)"""
        layers = (layers,) if isinstance(layers, str) else tuple(layers)
        shapes = {'rgb': ((n, height, width, 3), torch.uint8), 'depth': ((n, height, width), torch.float32), 'segmentation': ((n, height, width), torch.int32)}
        if not layers or any(k not in shapes for k in layers):
            raise ValueError('%s: layers are a non-empty choice of %s, not %r' % (who, sorted(shapes), layers))
        if depth not in ('buffer', 'metres'):
            raise ValueError("%s: depth is 'buffer' or 'metres', not %r" % (who, depth))
        if camera is not None and cameras is not None:
            raise ValueError('%s: camera or cameras, not both' % who)
        if not (float(near) > 0.0 and float(far) > float(near)):
            raise ValueError('%s: 0 < near < far, not near = %r, far = %r' % (who, near, far))
        if cameras is not None:
            if not (cameras.is_cuda and cameras.dtype == torch.float32 and tuple(cameras.shape) == (n, 11)):
                raise ValueError('%s: cameras is a float32 device tensor [%d, 11], not %s %s on %s' % (who, n, cameras.dtype, tuple(cameras.shape), cameras.device))
            cameras = cameras.contiguous()
        return layers, shapes, cameras

    def render_layers(self, width=200, height=200, envs=None, camera=None, cameras=None, layers=('rgb', 'depth', 'segmentation'), depth='buffer', near=0.01,
                      far=10.0, sub_goal=None, ghost_arm=None, out=None):
        """the layers of getCameraImage for envs [lo, hi) (default: all) as a dict of device tensors: 'rgb' uint8 [n, height, width, 3] (render's image, byte for
        byte), 'depth' float32 [n, height, width] (depth='buffer': PyBullet's depthBuffer in [0, 1] for near / far, 1 on a miss; 'metres': eye-space z, far on a
        miss), 'segmentation' int32 [n, height, width] (-1 on a miss, else collider | (link + 1) << 24: unpack_segmentation).  camera: an rp_camera for all envs
        (self.camera(...)), or cameras: a float32 device tensor [n, 11], one row per env (self.cameras(...)) - not both.  Ghosts (sub_goal, ghost_arm: as render's)
        tint rgb only.  out: a dict of preallocated tensors for some or all of the layers.  near / far shape the depth value only.  Nothing is read back."""
        lo, n, sub_goal, ghost_arm = self._render_args(envs, sub_goal, ghost_arm)
        width, height = int(width), int(height)
        layers, shapes, cameras = self._layer_args('render_layers', n, width, height, layers, depth, camera, cameras, near, far)
        res = {}
        for k in layers:
            shape, dtype = shapes[k]
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.is_cuda, (k, t.shape, t.dtype)
            res[k] = t
        self._call('rp_render_layers', _cam(camera), _ptr(cameras), float(near), float(far), _depth_mode(depth), width, height, lo, n, _ptr(res.get('rgb')),
                   _ptr(res.get('depth')), _ptr(res.get('segmentation')), _ptr(sub_goal), _ptr(ghost_arm), self._stream())
        return res

    POINTS_KEYS = ('n', 'frame', 'max_depth', 'drop', 'colour')

    def _points_spec(self, who, n, frame='world', max_depth=None, drop=()):
        """the host-side checks of a cloud's arguments (ValueError) and the rp_points_spec they make: n in 1 .. 65536, frame 'world' or 'camera', max_depth None
        (no limit) or a positive finite number of metres, drop a list of names from visual_names"""
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= _lib.MAX_POINTS:
            raise ValueError('%s: the number of points is an int in 1 .. %d, not %r' % (who, _lib.MAX_POINTS, n))
        if frame not in ('world', 'camera'):
            raise ValueError("%s: frame is 'world' or 'camera', not %r" % (who, frame))
        if max_depth is not None:
            try:
                ok = 0.0 < float(max_depth) < float('inf')
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError('%s: max_depth is None or a positive finite number of metres, not %r' % (who, max_depth))
        names = self.visual_names
        if isinstance(drop, str) or any(d not in names for d in drop):
            raise ValueError('%s: drop is a list of names from visual_names (%s), not %r' % (who, ', '.join(sorted(set(names))), drop))
        bits = 0
        for c, nm in enumerate(names):
            if nm in drop:
                bits |= 1 << c
        return _lib.RpPointsSpec(n, _lib.POINTS_CAMERA if frame == 'camera' else _lib.POINTS_WORLD, float(max_depth) if max_depth is not None else 0.0, bits)

    def _points_of_view(self, who, points, layers, depth):
        """the `points` key of set_image_obs / of a view of set_image_views: (rp_points_spec, colour) after its checks (ValueError, `who` names the call and the view)"""
        who = who + ': points'
        if not hasattr(points, 'keys') or set(points) - set(self.POINTS_KEYS) or 'n' not in points:
            raise ValueError('%s is a dict with n and optionally %s, not %r' % (who, ', '.join(self.POINTS_KEYS[1:]), points))
        colour = bool(points.get('colour', False))
        need = ('depth', 'segmentation') + (('rgb',) if colour else ())
        if depth != 'metres' or any(k not in layers for k in need):
            raise ValueError("%s need the layers %s with depth='metres'; the view has %r with depth=%r" % (who, need, layers, depth))
        return self._points_spec(who, points['n'], points.get('frame', 'world'), points.get('max_depth'), points.get('drop', ())), colour

    def _points_tensors(self, n, P, colour):
        """the output tensors of a cloud of P points for n envs"""
        t = {'xyz': torch.zeros((n, P, 3), dtype=torch.float32, device=self.device), 'segmentation': torch.zeros((n, P), dtype=torch.int32, device=self.device),
             'count': torch.zeros(n, dtype=torch.int32, device=self.device)}
        if colour:
            t['rgb'] = torch.zeros((n, P, 3), dtype=torch.uint8, device=self.device)
        return t

    @staticmethod
    def _points_ptrs(t):
        return [_ptr((t or {}).get(k)) for k in ('xyz', 'segmentation', 'rgb', 'count')]

    def render_points(self, width, height, n_points, envs=None, camera=None, cameras=None, frame='world', max_depth=None, drop=(), colour=False):
        """A fixed-size point cloud per env from one camera view (rp_render_points): the depth (metres) and segmentation layers of render_layers for envs [lo, hi)
        (default: all) with the same camera arguments, and their hits compacted on the device into P = n_points points, without a host wait.  Returns a dict of device
        tensors: 'xyz' float32 [n, P, 3], 'segmentation' int32 [n, P] (the pixel's packed value: unpack_segmentation), 'count' int32 [n], 'rgb' uint8 [n, P, 3] only
        with colour=True, and 'layers', the layers it drew ({'depth', 'segmentation'[, 'rgb']}).

        The rule: pixels in row-major order; a pixel is valid if its ray hit something (segmentation != -1), its collider is not among drop - a list of names from
        visual_names, e.g. the table or the ground plate - and its depth is <= max_depth (None: no limit).  With n valid pixels: n <= P keeps them all, in scan
        order, and slots n .. P - 1 are padding (xyz 0, segmentation -1, rgb 0); n > P keeps, in slot j, the valid pixel of rank floor(j n / P): an even,
        deterministic stride.  count is n itself, not capped: min(count, P) slots are real and count / P is the subsampling ratio.  frame='camera': (x, y, z) along
        the camera's right, up and forward axes, z the depth value bit for bit; 'world': eye + (forward + right nx + up ny) z with the basis the renderer used - for
        the gripper camera (camera=self.camera(gripper=True)) the basis at each env's EE link.  Host values are checked (ValueError)."""
        spec = self._points_spec('render_points', n_points, frame, max_depth, drop)
        lo, n, _, _ = self._render_args(envs, None, None)
        width, height = int(width), int(height)
        layers = ('depth', 'segmentation') + (('rgb',) if colour else ())
        layers, shapes, cameras = self._layer_args('render_points', n, width, height, layers, 'metres', camera, cameras, 0.01, 10.0)
        lay = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=self.device) for k in layers}
        pts = self._points_tensors(n, spec.max_points, colour)
        self._call('rp_render_points', _cam(camera), _ptr(cameras), width, height, lo, n, C.byref(spec), _ptr(lay.get('rgb')),
                   _ptr(lay['depth']), _ptr(lay['segmentation']), *self._points_ptrs(pts), self._stream())
        return {**pts, 'layers': lay}

    def render_states(self, states, width, height, index=None, visuals=None, camera=None, cameras=None, layers=('rgb', 'depth', 'segmentation'), depth='buffer',
                      near=0.01, far=10.0, goal=None, goal_mode='ghost', out=None):
        """render_layers for M images of states the envs need not be in (rp_render_states): a dict of device tensors 'rgb' uint8 [M, height, width, 3], 'depth'
        float32 [M, height, width], 'segmentation' int32 [M, height, width].  The live envs are neither written nor disturbed, and M is not bound to num_envs.

        states: a float32 device tensor [R, >= 128] whose last dimension is contiguous - a get_state() result, its [:, :128] slice (the state record is all that is
        read of a row), a view into a larger replay buffer; the row stride is states.stride(0).  None: the live envs' rows.  index: int32 device tensor [M], image i
        draws row index[i] (default: row i, M = R); an entry outside [0, R) leaves image i unwritten - its rows of `out` keep what they held.  visuals: None (the
        default look: baked colours, default light and background) or an int32 device tensor [M] of env indices: image i is drawn with set_visuals' row of env
        visuals[i]; an entry outside [0, num_envs) gives the default look.  camera / cameras ([M, 11], one row per image), layers, depth, near, far, out: as
        render_layers'; the gripper camera sits at the EE link of the row's state.

        goal: float32 [M, dims.achieved_goal] or None.  goal_mode='ghost': render_layers' sub_goal - half-transparent ghosts in rgb only.  'solid': the objects
        and, on play ids, drawer, door, button and dial are drawn AT the goal - opaque, in all three layers, the toggles coloured by the goal's joint values: the
        image of the row with the goal's words written into it.  Host values are checked (ValueError) before the library is touched; nothing is read back."""
        who = 'render_states'
        if states is not None:
            if not (torch.is_tensor(states) and states.dtype == torch.float32 and states.dim() == 2):
                raise ValueError('%s: states is None or a float32 tensor [R, >= 128], not %s' % (who, (states.dtype, tuple(states.shape)) if torch.is_tensor(states)
                                                                                                 else type(states).__name__))
            if states.shape[0] < 1 or states.shape[1] < 128:
                raise ValueError('%s: states has at least one row of at least 128 floats (the 512-byte state record), not %s' % (who, tuple(states.shape)))
            if states.stride(1) != 1 or states.stride(0) < 128:
                raise ValueError('%s: the last dimension of states is contiguous and its rows lie at least 128 floats apart, not strides %s' % (who, tuple(states.stride())))
            if not states.is_cuda:
                raise ValueError('%s: states is a device tensor, not one on %s' % (who, states.device))
        rows = self.num_envs if states is None else int(states.shape[0])
        for name, t in (('index', index), ('visuals', visuals)):
            if t is not None and not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1 and t.is_cuda):
                raise ValueError('%s: %s is None or an int32 device tensor [M], not %s' % (who, name, (t.dtype, tuple(t.shape), str(t.device)) if torch.is_tensor(t)
                                                                                           else type(t).__name__))
        m = rows if index is None else int(index.shape[0])
        if m < 1:
            raise ValueError('%s: no image to draw (index is empty)' % who)
        if visuals is not None and visuals.shape[0] != m:
            raise ValueError('%s: visuals has %d entries for %d images' % (who, visuals.shape[0], m))
        if goal_mode not in ('ghost', 'solid'):
            raise ValueError("%s: goal_mode is 'ghost' or 'solid', not %r" % (who, goal_mode))
        width, height = int(width), int(height)
        layers, shapes, cameras = self._layer_args(who, m, width, height, layers, depth, camera, cameras, near, far)
        if goal is not None:
            if not (torch.is_tensor(goal) and tuple(goal.shape) == (m, self.dims['achieved_goal'])):
                raise ValueError('%s: goal is a tensor [%d, %d], not %s' % (who, m, self.dims['achieved_goal'], tuple(goal.shape) if torch.is_tensor(goal) else type(goal).__name__))
            goal = goal.to(device=self.device, dtype=torch.float32).contiguous()
        res = {}
        for k in layers:
            shape, dtype = shapes[k]
            t = out.get(k) if out is not None else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=self.device)
            if not (tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.is_cuda):
                raise ValueError('%s: out[%r] is a contiguous %s device tensor %s, not %s %s' % (who, k, dtype, shape, t.dtype, tuple(t.shape)))
            res[k] = t
        index = index.contiguous() if index is not None else None
        visuals = visuals.contiguous() if visuals is not None else None
        src = _lib.RpStateRows(_ptr(states), 4 * states.stride(0) if states is not None else 0, rows, _ptr(index), _ptr(visuals))
        self._call('rp_render_states', C.byref(src), m, _cam(camera), _ptr(cameras), float(near), float(far), _depth_mode(depth), width, height, _ptr(res.get('rgb')),
                   _ptr(res.get('depth')), _ptr(res.get('segmentation')), _ptr(goal), _lib.GOAL_SOLID if goal_mode == 'solid' else _lib.GOAL_GHOST, self._stream())
        return res

    def goal_images(self, goal, width, height, camera=None, cameras=None, layers=('rgb', 'depth', 'segmentation'), depth='buffer', near=0.01, far=10.0, out=None):
        """every live env drawn AT its goal, with its own visuals: render_states(None, width, height, visuals=arange(num_envs), goal=goal, goal_mode='solid', ...) -
        the goal image a goal-conditioned pixel policy is given.  goal: [num_envs, dims.achieved_goal], e.g. obs['desired_goal']."""
        return self.render_states(None, width, height, visuals=torch.arange(self.num_envs, dtype=torch.int32, device=self.device), camera=camera, cameras=cameras,
                                  layers=layers, depth=depth, near=near, far=far, goal=goal, goal_mode='solid', out=out)

    @staticmethod
    def _image_keys(t):
        """the observation's image keys of a set_image_obs tensor dict: 'img' (the rgb tensor, None unless asked for), 'depth' and 'segmentation' where asked for"""
        return {'img': t.get('rgb'), **{k: t[k] for k in ('depth', 'segmentation') if k in t}}

    def _image_view(self, who, width, height, layers, camera, cameras, depth, near, far, terminal=True, points=None):
        """set_image_obs' and a view of set_image_views' host-side checks (ValueError; `who` names the call and the view) and tensors: (width, height, cameras, the
        zeroed observation tensors {layer: tensor}, the terminal ones - None without autoreset or with terminal=False)"""
        width, height = int(width), int(height)
        if cameras is not None and isinstance(cameras, torch.Tensor) and not cameras.is_contiguous():
            raise ValueError('%s: cameras must be contiguous (it is read in place at every draw)' % who)
        layers, shapes, cameras = self._layer_args(who, self.num_envs, width, height, layers, depth, camera, cameras, near, far)
        if not (0 < width <= 4096 and 0 < height <= 4096):
            raise ValueError('%s: width and height lie in 1 .. 4096, not %d x %d' % (who, width, height))
        if points is not None:
            self._points_of_view(who, points, layers, depth)      # (checked before anything changes; attached by the caller)

        def alloc():
            return {k: torch.zeros(shapes[k][0], dtype=shapes[k][1], device=self.device) for k in layers}
        return width, height, cameras, alloc(), alloc() if self.autoreset and terminal else None

    def set_image_obs(self, width=84, height=84, layers=('rgb',), camera=None, cameras=None, depth='buffer', near=0.01, far=10.0):
        """Camera images as part of the observation (rp_set_image_obs): from now on step, reset, reset(o=...) and calc_state draw the chosen layers of every env whose
        observation rows they write, inside the same library call and from the state those rows describe - byte for byte what render_layers(width, height, layers=...,
        same camera arguments) gives right after the call, without ghosts, with set_visuals' table.  obs['img'] is then the rgb tensor uint8 [N, height, width, 3] (None
        unless 'rgb' is among the layers), obs['depth'] float32 [N, height, width] and obs['segmentation'] int32 [N, height, width] exist where asked for.  A masked
        reset redraws the masked envs' rows only.  With autoreset=True, obs holds an ended env's first frame of the new episode and info['terminal_observation'] gets
        the same keys with the ended envs' LAST frame, drawn between the step and the reset (rows valid where done; the others keep what they held).  All these tensors
        are owned like buf: the next call overwrites them (clone to keep).

        camera: an rp_camera for all envs (self.camera(...), gripper=True included; None: the reference's fixed camera), or cameras: a float32 device tensor [N, 11]
        (self.cameras(...)), kept as self.image_cameras and read on the device at every draw, so rows may be rewritten in place between calls (a new camera per
        episode: image_cameras[done] = ...).  depth / near / far as render_layers'.  Host values are checked as render_layers checks them (ValueError).  While set,
        record_images' 200 x 200 render is not made.  set_image_obs(None) switches the feature off: obs['img'] is None, or record_images' picture, again.  Switching on,
        over or off may synchronise the device; the configuration is not part of get_state / set_state / clone_envs.

        set_image_points(...) afterwards attaches a point cloud to this view: obs['points'].  This call, like set_image_views, drops a cloud attached before."""
        if width is None:
            self._call('rp_set_image_obs', None, None, 0.0, 0.0, 0, 0, 0, None, None, None, None, None, None)
            self._no_images()
            return
        width, height, cameras, obs, final = self._image_view('set_image_obs', width, height, layers, camera, cameras, depth, near, far)
        ptrs = [_ptr(t.get(k)) for t in (obs, final or {}) for k in ('rgb', 'depth', 'segmentation')]
        self._call('rp_set_image_obs', _cam(camera), _ptr(cameras), float(near), float(far), _depth_mode(depth), width, height, *ptrs)
        self._no_images()      # (the handle has one image configuration: this call replaced set_image_views' too)
        self.image_obs, self.image_final, self.image_cameras, self._image_depth = obs, final, cameras, depth
        self._kept['rp_set_image_obs'] = (obs, final, cameras)      # (kept until the next set: the library writes and reads them at every draw)

    def set_image_points(self, n, frame='world', max_depth=None, drop=(), colour=False, view=None):
        """A point cloud of n points per env as part of the observation (rp_set_image_points), attached to the image configuration in force: to set_image_obs' view
        (view=None), or to the view of set_image_views that `view` names - where the same arguments can be given as that view's points=dict(n=..., frame=...,
        max_depth=..., drop=..., colour=...).  The view must list 'depth' with depth='metres' and 'segmentation', plus 'rgb' for colour; a ValueError names the view.
        From now on every call that draws the view compacts its hits by one more launch behind the draw - one launch for all clouds of a pass -, by render_points' rule
        and with its arguments (drop takes names from visual_names): where an env's view has more valid pixels than points, slot j holds the valid pixel of rank
        floor(j n / P) (n valid pixels, P points), and otherwise all of them in scan order followed by padding (xyz 0, segmentation -1, rgb 0); count is the
        number of valid pixels, not capped.  obs['points'] (set_image_obs) or obs['views'][name]['points'] is {'xyz' float32 [N, P, 3], 'segmentation' int32 [N, P], 'count' int32 [N]
        [, 'rgb' uint8 [N, P, 3]]}, each row what render_points gives for that env at that moment; a masked reset rewrites the masked envs' rows only.  With
        autoreset=True, and terminal frames on the view, info['terminal_observation'] carries the same keys at the same place for the ended envs' last frame (rows
        valid where done).  The tensors are owned like buf.  n=None detaches the cloud; any later set_image_obs or set_image_views drops every cloud."""
        if self.image_views is not None:
            if view not in self.image_views:
                raise ValueError('set_image_points: view is one of %s, not %r' % (', '.join(repr(k) for k in self.image_views), view))
            who, index, obs, final = 'set_image_points: view %r' % (view,), list(self.image_views).index(view), self.image_views[view], (self.image_views_final or {}).get(view)
            depth = self._image_depth[view]
        elif self.image_obs is not None:
            if view is not None:
                raise ValueError('set_image_points: view names a view of set_image_views; set_image_obs\' view is view=None, not %r' % (view,))
            who, index, obs, final, depth = 'set_image_points', 0, self.image_obs, self.image_final, self._image_depth
        else:
            raise ValueError('set_image_points: no image configuration is in force (set_image_obs or set_image_views first)')
        if n is None:
            self._call('rp_set_image_points', index, None, *[None] * 8)
            self._set_points(view, None, None)
            return
        spec, colour = self._points_of_view(who, dict(n=n, frame=frame, max_depth=max_depth, drop=drop, colour=colour), [k for k in obs if k != 'points'], depth)
        pts = self._points_tensors(self.num_envs, spec.max_points, colour)
        fpts = self._points_tensors(self.num_envs, spec.max_points, colour) if final is not None else None
        self._call('rp_set_image_points', index, C.byref(spec), *self._points_ptrs(pts), *self._points_ptrs(fpts))
        self._set_points(view, pts, fpts)

    def _set_points(self, view, pts, fpts):
        """the cloud tensors of a view (None: gone) where the observation finds them; the library holds the same pointers"""
        self._kept.setdefault('rp_set_image_points', {})[view] = (pts, fpts)      # (kept until the configuration goes: the library writes them at every draw)
        if self.image_views is None:
            self.image_points, self.image_points_final = pts, fpts
            return
        for t, c in ((self.image_views[view], pts), ((self.image_views_final or {}).get(view), fpts)):
            if t is not None:
                t.pop('points', None)
                if c is not None:
                    t['points'] = c

    def _no_images(self):
        """forget the tensors of the image configuration the library has just dropped (set_image_obs' or set_image_views': the handle holds one)"""
        self.image_obs = self.image_final = self.image_cameras = None
        self.image_points = self.image_points_final = self._image_depth = None
        self.image_views = self.image_views_final = None
        self._kept.pop('rp_set_image_points', None)
        self.image_view_cameras = {}
        self._kept.pop('rp_set_image_obs', None)

    def set_image_views(self, views):
        """Several camera views per env as part of the observation (rp_set_image_views): views is an ordered mapping of 1 to 4 names to dicts of set_image_obs' keyword
        arguments (width, height, layers, camera, cameras, depth, near, far; set_image_obs' defaults), e.g. {'img': dict(width=84, height=84), 'wrist': dict(width=64,
        height=64, layers=('rgb', 'depth'), camera=env.camera(gripper=True))}.  From now on step, reset, reset(o=...) and calc_state draw every view of the envs whose
        observation rows they write, inside the same library call - with two or more views one pose launch and one draw launch for all of them -, each view byte for
        byte what render_layers gives with that view's arguments.  obs['views'][name] is {layer: tensor}; obs['img'] is the rgb tensor of the view named 'img' if there
        is one, else None; obs['depth'] / obs['segmentation'] are absent.  With autoreset=True info['terminal_observation']['views'] has the same shape with the ended
        envs' last frames (rows valid where done); a view given terminal=False has no terminal tensors and is left out of the terminal pass.  Host values are checked
        per view as set_image_obs checks them; a ValueError names the view.  self.image_view_cameras[name] is the per-env camera tensor of a view that has one: rows
        may be rewritten in place between calls.  While set, record_images' 200 x 200 render is not made.  The handle has ONE image configuration: set_image_views
        replaces set_image_obs' and the reverse; set_image_views(None) and set_image_obs(None) both switch it off.

        A view's dict may carry set_image_points' arguments as points=dict(n=..., frame=..., max_depth=..., drop=..., colour=...): obs['views'][name]['points'] is then that view's
        cloud {'xyz', 'segmentation', 'count'[, 'rgb']}, and with terminal frames info['terminal_observation']['views'][name]['points'] the ended envs'.  All clouds of
        a pass are compacted by ONE more launch behind the draw.  A view without points has exactly the keys it has without the feature."""
        if views is None:
            self._call('rp_set_image_views', None, 0)
            self._no_images()
            return
        if not hasattr(views, 'items') or not 1 <= len(views) <= _lib.MAX_IMAGE_VIEWS:
            raise ValueError('set_image_views: views is a mapping of 1 to %d names to dicts of set_image_obs\' arguments' % _lib.MAX_IMAGE_VIEWS)
        arr = (_lib.RpImageView * len(views))()
        obs, final, cams, depths, keep = {}, {}, {}, {}, []
        defaults = dict(width=84, height=84, layers=('rgb',), camera=None, cameras=None, depth='buffer', near=0.01, far=10.0, terminal=True, points=None)
        for i, (name, kw) in enumerate(views.items()):
            who = 'set_image_views: view %r' % (name,)
            if not hasattr(kw, 'keys') or set(kw) - set(defaults):
                raise ValueError('%s: a dict with keys among %s, not %r' % (who, sorted(defaults), kw))
            a = {**defaults, **kw}
            width, height, cameras, obs[name], fin = self._image_view(who, **a)
            depths[name] = a['depth']
            if fin is not None:
                final[name] = fin
            if cameras is not None:
                cams[name] = cameras
            v = arr[i]
            if a['camera'] is not None:
                keep.append(a['camera'])
                v.cam = C.pointer(a['camera'])
            v.cam_rows = cameras.data_ptr() if cameras is not None else None
            v.near_plane, v.far_plane, v.depth_mode, v.width, v.height = float(a['near']), float(a['far']), _depth_mode(a['depth']), width, height
            for prefix, tensors in (('', obs[name]), ('final_', fin or {})):
                for k, t in tensors.items():
                    setattr(v, prefix + k, t.data_ptr())
        self._call('rp_set_image_views', arr, len(views))
        self._no_images()
        self.image_views, self.image_views_final, self.image_view_cameras, self._image_depth = obs, (final if self.autoreset else None), cams, depths
        self._kept['rp_set_image_obs'] = (obs, final, cams)      # (the one image configuration's tensors, kept until the next set or switch-off)
        for name, kw in views.items():
            if kw.get('points') is not None:
                self.set_image_points(view=name, **kw['points'])

    def ray_test(self, ray_from, ray_to):
        """bullet_client.rayTest for k rays per env: ray_from / ray_to [N, k, 3] (world).  Returns dict(hit_fraction [N, k] (1 = miss),
        collider [N, k] (-1 = miss), link [N, k] (Bullet link index of an arm collider, else -1), hit_position, hit_normal [N, k, 3])"""
        f = ray_from.to(device=self.device, dtype=torch.float32).contiguous()
        t = ray_to.to(device=self.device, dtype=torch.float32).contiguous()
        assert f.shape == t.shape and f.dim() == 3 and f.shape[0] == self.num_envs and f.shape[2] == 3, f.shape
        k = f.shape[1]
        out = {'hit_fraction': torch.empty((self.num_envs, k), dtype=torch.float32, device=self.device),
               'collider': torch.empty((self.num_envs, k), dtype=torch.int32, device=self.device),
               'link': torch.empty((self.num_envs, k), dtype=torch.int32, device=self.device),
               'hit_position': torch.empty((self.num_envs, k, 3), dtype=torch.float32, device=self.device),
               'hit_normal': torch.empty((self.num_envs, k, 3), dtype=torch.float32, device=self.device)}
        self._call('rp_ray_test', _ptr(f), _ptr(t), k, _ptr(out['hit_fraction']), _ptr(out['collider']), _ptr(out['link']), _ptr(out['hit_position']),
                   _ptr(out['hit_normal']), self._stream())
        return out

    @property
    def collider_names(self):
        """one unique name per collider, in collider order: the collider numbers of closest_points' pairs and of ray_test's answer (an object with several colliders:
        'drawer.0' .. 'drawer.9'; an arm collider: its link, 'link7')"""
        return collider_names(MODEL_OF[self.env_id])

    def _colliders_of(self, who, x):
        """the collider numbers one argument of collider_pairs names: an index, a name of collider_names, a name of visual_names (every collider of that object), or a
        sequence of those"""
        names, objects = self.collider_names, self.visual_names
        if isinstance(x, (str, int)) and not isinstance(x, bool):
            x = [x]
        out = []
        try:
            items = list(x)
        except TypeError:
            items = [x]
        for it in items:
            if isinstance(it, str):
                hit = [names.index(it)] if it in names else [c for c, o in enumerate(objects) if o == it]
                if not hit:
                    raise ValueError('%s: no collider or object is called %r (collider_names: %s)' % (who, it, ', '.join(names)))
                out += hit
            elif isinstance(it, int) and not isinstance(it, bool):
                if not 0 <= it < len(names):
                    raise ValueError('%s: collider %d lies outside 0 .. %d' % (who, it, len(names) - 1))
                out.append(it)
            else:
                raise ValueError('%s: a collider is a name or an index, not %r' % (who, it))
        return out

    def collider_pairs(self, a, b, group=0):
        """the pair list of closest_points: an int32 device tensor [K, 3] of rows (collider a, collider b, group) - the full product of the colliders `a` names with
        those `b` names, a-major, without the pairs of a collider with itself.  a, b: a name of collider_names, an object's name from visual_names (every collider of
        the object), an index, or a sequence of those.  Lists of several groups: torch.cat."""
        who = 'collider_pairs'
        if isinstance(group, bool) or not isinstance(group, int) or not 0 <= group < _lib.CP_MAX_GROUPS:
            raise ValueError('%s: group is an integer in 0 .. %d, not %r' % (who, _lib.CP_MAX_GROUPS - 1, group))
        ca, cb = self._colliders_of(who, a), self._colliders_of(who, b)
        rows = [(x, y, group) for x in ca for y in cb if x != y]
        if not rows:
            raise ValueError('%s: no pair is left (a and b name the same single collider)' % who)
        return torch.tensor(rows, dtype=torch.int32, device=self.device).reshape(-1, 3)

    def closest_points(self, pairs, states=None, index=None, max_distance=None, n_groups=0, out=None):
        """bullet_client.getClosestPoints for K collider pairs of every live env or of stored state rows (rp_closest_points): a dict of device tensors 'distance'
        float32 [M, K], 'point_a' / 'point_b' / 'normal' float32 [M, K, 3] (world; the normal from b toward a) and 'status' int32 [M, K]; with n_groups = G > 0 also
        'group_min' float32 [M, G] and 'group_pair' int32 [M, G].  The shapes are the ray caster's, without margins: exact boxes, spheres, the links' convex hulls.

        status: 0 separated (distance > 0, point_a - point_b = normal * distance); 1 overlap or touching (distance exactly 0, both points the common point, normal
        zero - penetration depth is not reported); 2 far (only with max_distance > 0: the gap of the world boxes around the shapes exceeds it; distance =
        max_distance, points and normal zero); 3 skipped (a collider number outside the model, a == b, or a bad row index: the pair's other outputs keep what they
        held - zero in tensors made here); bit 4: the bounded iteration ended at its cap, the distance is an upper bound.

        pairs: collider_pairs(...) - an int32 device tensor [K, 3] of (collider a, collider b, group), passed through unread - or a host list of such triples (or of
        (a, b) pairs: group 0), which is range-checked here; 1 <= K <= 4096.  group_min / group_pair: per row and group the smallest distance over the group's pairs
        that are not skipped (a far pair counts with max_distance) and that pair's index, the lowest among equals; +inf / -1 for an empty group.
        states / index: as render_states' - a float32 device tensor [R, >= 128] of get_state() rows and an int32 device tensor [M] of rows to take (an entry outside
        [0, R): every pair of that row is skipped); None: the live envs.  max_distance: None or <= 0: no cut.  out: a dict of tensors to write into (SKIPPED cells keep
        their values).  Host values are checked (ValueError) before the library is touched; nothing is read back; the live envs are neither written nor disturbed."""
        who = 'closest_points'
        if torch.is_tensor(pairs) and pairs.is_cuda:
            if not (pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 3):
                raise ValueError('%s: pairs is an int32 tensor [K, 3], not %s %s' % (who, pairs.dtype, tuple(pairs.shape)))
            pairs = pairs.contiguous()
        else:
            try:
                rows = [[int(v) for v in p] for p in (pairs.tolist() if torch.is_tensor(pairs) else pairs)]
            except (TypeError, ValueError):
                raise ValueError('%s: pairs is an int32 device tensor [K, 3] or a list of (a, b) / (a, b, group), not %r' % (who, type(pairs).__name__)) from None
            n_col = len(self.collider_names)
            for p in rows:
                if len(p) == 2:
                    p.append(0)
                if len(p) != 3:
                    raise ValueError('%s: a pair is (a, b) or (a, b, group), not %r' % (who, tuple(p)))
                if not (0 <= p[0] < n_col and 0 <= p[1] < n_col) or p[0] == p[1]:
                    raise ValueError('%s: pair %r: colliders lie in 0 .. %d and differ' % (who, tuple(p[:2]), n_col - 1))
                if not 0 <= p[2] < max(int(n_groups) if isinstance(n_groups, int) else 0, 1):
                    raise ValueError('%s: pair %r: group %d lies outside 0 .. %d' % (who, tuple(p[:2]), p[2], max(int(n_groups), 1) - 1))
            pairs = torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)
        k = int(pairs.shape[0])
        if not 1 <= k <= _lib.CP_MAX_PAIRS:
            raise ValueError('%s: pairs has %d rows, expected 1 .. %d' % (who, k, _lib.CP_MAX_PAIRS))
        if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 0 <= n_groups <= _lib.CP_MAX_GROUPS:
            raise ValueError('%s: n_groups is an integer in 0 .. %d, not %r' % (who, _lib.CP_MAX_GROUPS, n_groups))
        if max_distance is None:
            max_distance = 0.0
        try:
            max_distance = float(max_distance)
        except (TypeError, ValueError):
            raise ValueError('%s: max_distance is None or a number of metres, not %r' % (who, max_distance)) from None
        if max_distance != max_distance:
            raise ValueError('%s: max_distance is None or a number of metres, not NaN' % who)
        if states is not None:
            if not (torch.is_tensor(states) and states.dtype == torch.float32 and states.dim() == 2):
                raise ValueError('%s: states is None or a float32 tensor [R, >= 128], not %s' % (who, (states.dtype, tuple(states.shape)) if torch.is_tensor(states)
                                                                                                 else type(states).__name__))
            if states.shape[0] < 1 or states.shape[1] < 128:
                raise ValueError('%s: states has at least one row of at least 128 floats (the 512-byte state record), not %s' % (who, tuple(states.shape)))
            if states.stride(1) != 1 or states.stride(0) < 128:
                raise ValueError('%s: the last dimension of states is contiguous and its rows lie at least 128 floats apart, not strides %s' % (who, tuple(states.stride())))
            if not states.is_cuda:
                raise ValueError('%s: states is a device tensor, not one on %s' % (who, states.device))
        n_rows = self.num_envs if states is None else int(states.shape[0])
        if index is not None and not (torch.is_tensor(index) and index.dtype == torch.int32 and index.dim() == 1 and index.is_cuda):
            raise ValueError('%s: index is None or an int32 device tensor [M], not %s' % (who, (index.dtype, tuple(index.shape), str(index.device)) if torch.is_tensor(index)
                                                                                          else type(index).__name__))
        m = n_rows if index is None else int(index.shape[0])
        if m < 1:
            raise ValueError('%s: no row to query (index is empty)' % who)
        shapes = {'distance': ((m, k), torch.float32), 'point_a': ((m, k, 3), torch.float32), 'point_b': ((m, k, 3), torch.float32),
                  'normal': ((m, k, 3), torch.float32), 'status': ((m, k), torch.int32)}
        if n_groups > 0:
            shapes.update({'group_min': ((m, n_groups), torch.float32), 'group_pair': ((m, n_groups), torch.int32)})
        if out is not None and (not isinstance(out, dict) or set(out) - set(shapes)):
            raise ValueError('%s: out is a dict with keys among %s' % (who, ', '.join(shapes)))
        for key, t in (out or {}).items():
            shape, dtype = shapes[key]
            if t is not None and not (torch.is_tensor(t) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.is_cuda):
                raise ValueError('%s: out[%r] is a contiguous %s device tensor %s, not %s' % (who, key, dtype, shape, (t.dtype, tuple(t.shape), str(t.device))
                                                                                             if torch.is_tensor(t) else type(t).__name__))
        res = {}
        for key, (shape, dtype) in shapes.items():
            t = out.get(key) if out is not None else None
            res[key] = t if t is not None else torch.zeros(shape, dtype=dtype, device=self.device)
        pairs = pairs.to(self.device)
        index = index.contiguous() if index is not None else None
        src = _lib.RpStateRows(_ptr(states), 4 * states.stride(0) if states is not None else 0, n_rows, _ptr(index), None)
        self._call('rp_closest_points', C.byref(src), m, _ptr(pairs), k, n_groups, max_distance, _ptr(res['distance']), _ptr(res['point_a']), _ptr(res['point_b']),
                   _ptr(res['normal']), _ptr(res['status']), _ptr(res.get('group_min')), _ptr(res.get('group_pair')), self._stream())
        self._kept['rp_closest_points'] = (pairs, index, states)      # (kept until the next call: the kernel reads them when the stream gets there)
        return res

    def get_state(self):
        n = self.lib.rp_state_bytes(self.h) // 4
        s = torch.empty((self.num_envs, n), dtype=torch.float32, device=self.device)
        self._call('rp_get_state', _ptr(s), self._stream())
        return s

    def set_state(self, s):
        """s: [N or 1, rp_state_bytes / 4] as get_state returns it - or only the state records ([.., 128], e.g. built from an oracle's state): the envs then
        start without contact history (an all-zero contact cache)"""
        s = s.to(device=self.device, dtype=torch.float32)
        if s.dim() == 1:
            s = s[None]
        n = self.lib.rp_state_bytes(self.h) // 4
        if s.shape[1] < n:
            s = torch.cat([s, torch.zeros((s.shape[0], n - s.shape[1]), dtype=torch.float32, device=self.device)], 1)
        s = s.contiguous()
        self._call('rp_set_state', _ptr(s), s.shape[0], self._stream())

    def replay(self, o0, actions, keys=('obs_quat', 'achieved_goal')):
        """Play recorded trajectories back (the reference's README use: "playing out the teleop data", "reset the environment to
        specific locations"): every env is placed from its first recorded observation o0[e] with reset(o) - objects and arm from
        the observation vector, nothing settles - then the recorded actions [T, N, action] are stepped open loop.  Returns
        {key: [T + 1, N, dim]} (index 0 = after the reset) plus 'reward' and 'is_success' [T, N]."""
        obs = self.reset(o=o0)
        out = {k: [obs[k].clone()] for k in keys}
        rew, suc = [], []
        for t in range(actions.shape[0]):
            obs, r, _, info = self.step(actions[t])
            for k in keys:
                out[k].append(obs[k].clone())
            rew.append(r.clone())
            suc.append(info['is_success'].clone())
        res = {k: torch.stack(v) for k, v in out.items()}
        res['reward'] = torch.stack(rew) if rew else torch.zeros((0, self.num_envs), device=self.device)
        res['is_success'] = torch.stack(suc) if suc else torch.zeros((0, self.num_envs), dtype=torch.int32, device=self.device)
        return res

    def set_fused(self, mode=1):
        """step pipeline: 0 = default (k_action, k_prep2, k_solve2, k_calc_state), 1 = one fused kernel per step (the
        library's in-GPU cross-check path).  Both are bit-identical."""
        self._call('rp_set_fused', int(mode))

    def set_groups(self, groups):
        """number of env groups (each with its own stream and kernel chain) rp_step uses; results do not depend on it"""
        self._call('rp_set_groups', int(groups))

    def set_debug_flags(self, flags):
        """test hook: bit 0 makes the solver give every contact its own folded slot (its fallback layout) instead of solving
        arm-only and non-arm contacts side by side; results are bit-identical either way"""
        self._call('rp_set_debug_flags', int(flags))

    def debug_row_counts(self):
        """test hook: per env of the latest substep, [unit rows, contacts, 1 if a contact in the arm's half of the velocity layout (arm links, and the
        rotation-locked drawer where the model has one: it rests on its rails), spanning contacts] (host tensor)"""
        buf = (C.c_int32 * (2 * self.num_envs))()
        self._call('rp_debug_row_counts', buf)
        a = torch.tensor(list(buf), dtype=torch.int64).reshape(self.num_envs, 2)
        return torch.stack([a[:, 0], a[:, 1] % 1000, (a[:, 1] // 1000) % 100, a[:, 1] // 100000], 1)

    def enable_timers(self, steps=64):
        """keep per-launch hipEvent timings for the next `steps` rp_step calls (0 disables)"""
        self._call('rp_enable_timers', int(steps))

    def timers(self):
        t = _lib.RpTimers()
        self._call('rp_get_timers', C.byref(t))
        return {n: getattr(t, n) for n, _ in _lib.RpTimers._fields_}

    def debug_action(self, actions, places=False):
        """test hook: the action stage alone on the current state (rp_debug_action).  Returns (raw [N, 7] float32: the joint solution before the clamps to the joint
        limits and to q +- inc, flags [N] int32: 1 = the last IK call ran out of iterations (status bit 8), 2 = a stopping test was marginal (bit 16)) and, with
        places=True, every env's place [N] int32 in the member table the launch went by; the motor targets and the status word are left in the state as a step
        leaves them (get_state)."""
        a = actions.to(device=self.device, dtype=torch.float32).contiguous()
        assert a.shape == (self.num_envs, self.dims['action']), a.shape
        raw = torch.empty((self.num_envs, 8), dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()      # (the hook runs on the NULL stream)
        self._call('rp_debug_action', _ptr(a), _ptr(raw))
        word = raw[:, 7].to(torch.int32)
        return (raw[:, :7].contiguous(), word & 3) + ((word >> 2,) if places else ())

    def debug_substep(self, env=0):
        buf = (C.c_float * 4096)()
        self._call('rp_debug_substep', env, buf)
        return torch.tensor(list(buf))
