"""The camera cases and their float64 reference, shared by tests/test_camera_cases.py (CPU: the table alone) and tests/test_gpu_camera_cases.py (the device against it).

Every picture the library draws is a ray cast over its collider table, so its reference is the same ray cast in numpy float64 over the CPU oracle's collider poses:
cast() below (boxes, spheres, and for the arm's links the convex hulls scipy builds from the oracle's hull vertices), with the rays of pixel_rays().  cast, cast_hull,
hull_planes, oracle_hulls, LIGHT, BACKGROUND and pixel_rays were written for tests/test_gpu_render.py and tests/test_gpu_render_layers.py, which import them from here now;
their arithmetic is unchanged.

ids      UR5PlayAbsRPY1Obj-v0 (model U), pandaPlayAbsRPY1Obj-v0 (V: the Panda's hulls), pandaPlay-v0 (W: the wide record, two objects)
states   built on the oracle (reset(), then set_state on its vector) and carried to the device with tools/gpu_debug.py's record_from_oracle + VecPlayEnv.set_state, so that
         both sides hold the same numbers: 'reset'; 'arm' (every arm joint moved by 0.2 to 0.6 rad, the gripper half open); 'scene' (drawer -0.06, door 0.12, button 0.01,
         dial 1.5 - the toggles recolour the globe and the grill -, the block lifted 8 cm and turned by a quaternion with no zero component); 'grip_pi', 'grip_a',
         'grip_b' (EE orientations for the gripper camera, GRIPPER_JOINTS).  record_from_oracle / oracle_state_from_record know the narrow record only, so the wide id
         is used at its reset state alone, device and oracle reset with equal seeds (env e of the handle = the oracle with env_index e).
cameras  CAMERAS; 'rows' = three per-env rows (ROWS) that differ in yaw, distance, fov and aspect
sizes    70 x 45 and 33 x 50 (ragged 16 x 16 tiles on both axes, non-square both ways); 200 x 200 for the UR5's gripper camera only

python tests/camera_cases.py prints one line per case (profiles/camera_cases_cpu.txt): the reference's own spread between the fp32 and the fp64 oracle, the hit share, the
colliders in view and, for the gripper cases, the EE's Euler angles and how far the link-frame basis (-z, +x) lies from the reference's."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'oracle')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LIGHT = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
BACKGROUND = np.array([0.82, 0.88, 0.96])
F32 = np.float32
PI = np.pi

U, V, W2 = 'UR5PlayAbsRPY1Obj-v0', 'pandaPlayAbsRPY1Obj-v0', 'pandaPlay-v0'
IDS = (U, V, W2)
SEEDS = {U: 4, V: 3, W2: 2}
NUM_ENVS = 3
SIZES = ((70, 45), (33, 50))                   # (width, height)
GRIPPER_SIZE_UR5 = (200, 200)
STATES = {U: ('reset', 'arm', 'scene'), V: ('reset', 'arm', 'scene'), W2: ('reset',)}
GRIPPER_STATES = ('reset', 'grip_pi', 'grip_a', 'grip_b')
CAMERAS = {'default': dict(),
           'wide43': dict(distance=2.0, yaw=20.0, pitch=-40.0, fov=60.0, aspect=4.0 / 3.0),
           'tall': dict(aspect=0.5, fov=35.0),
           'fov170': dict(target='edge', distance=0.6, fov=170.0),                     # as test_gpu_render_layers.make_camera has them
           'close': dict(target='block', distance=0.25, yaw=40.0, pitch=-15.0),       # (make_camera's 9 cm from the block shows 3 to 5 colliders: fewer than a case must)
           'gripper': dict(gripper=True)}
ROWS = dict(yaw=[-30.0, 20.0, 75.0], distance=[1.3, 2.0, 0.8], fov=[50.0, 60.0, 35.0], aspect=[1.0, 4.0 / 3.0, 0.6])
CAMERA_NAMES = tuple(CAMERAS) + ('rows',)
NEAR, FAR = 0.01, 10.0
SEG_CAP = 0.995                                # share of the pixels whose segmentation the device must get right (the existing render tests' cap)
SPREAD_CAP = 0.002                             # ... and what the reference itself may use of the 0.005 left
GRAZE = 0.02                                   # |n . d| below which a hit's depth is not held to 2e-4 m
DEPTH_TOL = 2e-4

# sub-goal ghosts: {id: {entry: (index into the achieved goal, value, added to the state's own value or absolute)}}; every entry is also moved alone
GHOST_SIZE = (200, 200)                        # at the default camera the button's ghost, 1.2 mm under its body, still shows on three pixels
GHOST_ENTRIES = {U: {'block': (0, 0.12, True), 'drawer': (7, -0.05, False), 'door': (8, 0.1, False), 'button': (9, 0.01, False), 'dial': (10, 0.8, False)},
                 V: {'block': (0, -0.1, True)},
                 W2: {'first': (0, 0.1, True), 'second': (7, 0.1, True), 'drawer': (14, -0.05, False), 'door': (15, 0.1, False)}}
GHOST_COMBINED = {U: ('block', 'drawer', 'door', 'button', 'dial'), V: ('block',), W2: ('second',)}          # the sub-goals drawn as a whole
GHOST_ARM_OFFSET = [0.15, 0.0, 0.05]           # the Panda's ghost arm: the EE pose moved by this, gripper 0

# arm joints (then the gripper's) of the states that move the arm.  'arm': the reset joints plus these; grip_*: absolute joints, found once with the oracle's IK for EE
# orientations with the Euler angles the gripper camera needs (roll near pi; |roll| between 0.3 and 2.5 with pitch and yaw away from 0) and rounded to 4 digits
ARM_DELTA = {'ur5': [0.3, 0.25, -0.35, 0.4, -0.5, 0.6], 'panda': [0.3, 0.25, -0.4, 0.35, 0.5, -0.3, 0.6]}
GRIPPER_HALF = {'ur5': [0.4, 0.4, 0.4, 0.4, 0.0224, 0.0224], 'panda': [0.02, 0.02]}
GRIPPER_JOINTS = {}                            # filled below: {(arm, state): joints}


def arm_of(gid):
    return 'panda' if gid.startswith('panda') else 'ur5'


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the ray cast (moved here from tests/test_gpu_render.py, unchanged)

def hull_planes(verts):
    """face planes (n [m, 3], w [m]: n . x + w <= 0 inside) of the convex hull of world-frame vertices - scipy's qhull on the vertices themselves, independent of the
    library's baked plane tables (tools/bake_hull_planes.py) and of its body -> collider frame change"""
    from scipy.spatial import ConvexHull
    eq = ConvexHull(verts).equations
    return eq[:, :3], eq[:, 3]


def cast_hull(planes, o, d, tmax):
    """rays against a convex polytope: enter = the latest plane crossed inwards, exit = the earliest crossed outwards; a ray that starts inside reports no hit"""
    nn, w = planes
    den = d @ nn.T                                     # [rays, planes]
    num = -(o @ nn.T + w)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = num / den
    par = np.abs(den) < 1e-12
    miss_par = (par & (num < 0)).any(axis=1)
    t_in = np.where((den < 0) & ~par, t, -np.inf)
    t_out = np.where((den > 0) & ~par, t, np.inf)
    k = t_in.argmax(axis=1)
    tin, tout = t_in.max(axis=1), np.minimum(t_out.min(axis=1), tmax)
    hit = (~miss_par) & (tin > 0) & (tin <= tout)
    return hit, tin, nn[k]


def cast(R, p, tab, o, d, tmax, hulls=None):
    """nearest hit of rays o + t d (t in [0, tmax]) against the colliders: (t [n], collider [n], normal [n, 3]); numpy float64.  hulls: {collider: planes} - the arm's
    links are the convex hulls of their collision meshes (what they collide as), everything else its box / sphere"""
    n = o.shape[0]
    best = np.full(n, np.inf)
    who = np.full(n, -1)
    nrm = np.zeros((n, 3))
    for c in range(len(tab)):
        he = tab[c, 1:4]
        if hulls and c in hulls:
            hit, t, nn = cast_hull(hulls[c], o, d, tmax)
        elif tab[c, 0] == 0:
            ol = (o - p[c]) @ R[c]
            dl = d @ R[c]
            inside = (np.abs(ol) <= he).all(axis=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                t1 = (-he - ol) / dl
                t2 = (he - ol) / dl
            lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
            par = np.abs(dl) < 1e-12
            lo = np.where(par, -np.inf, lo)
            hi = np.where(par, np.inf, hi)
            miss_par = (par & (np.abs(ol) > he)).any(axis=1)
            tmin = np.maximum(lo.max(axis=1), 0.0)
            tm = np.minimum(hi.min(axis=1), tmax)
            hit = (~inside) & (~miss_par) & (tmin <= tm)
            axis = np.where(lo.max(axis=1) > 0, lo.argmax(axis=1), 0)
            sgn = np.where(np.take_along_axis(t1, axis[:, None], 1)[:, 0] > np.take_along_axis(t2, axis[:, None], 1)[:, 0], 1.0, -1.0)
            nn = R[c][:, axis].T * sgn[:, None]
            t = tmin
        else:
            oc = o - p[c]
            a = (d * d).sum(1)
            b = 2 * (oc * d).sum(1)
            cc = (oc * oc).sum(1) - he[0] ** 2
            disc = b * b - 4 * a * cc
            with np.errstate(invalid='ignore'):
                t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            hit = (cc >= 0) & (disc >= 0) & (t >= 0) & (t <= tmax)
            nn = (oc + d * t[:, None]) / he[0]
        better = hit & (t < best)
        best = np.where(better, t, best)
        who = np.where(better, c, who)
        nrm = np.where(better[:, None], nn, nrm)
    return best, who, nrm


def oracle_hulls(orc):
    R, p, tab = orc.colliders()
    out = {}
    for c in range(len(tab)):
        v = orc.hull_vertices(c)
        if v is not None:
            out[c] = hull_planes(v)
    return out


def hull_spheres(orc):
    """{collider: (centre, radius)} of a ball around each hull's vertices"""
    out = {}
    for c in range(len(orc.colliders()[2])):
        v = orc.hull_vertices(c)
        if v is not None:
            out[c] = (v.mean(axis=0), np.linalg.norm(v - v.mean(axis=0), axis=1).max())
    return out


NO_HULL = (np.zeros((1, 3)), np.ones(1))          # a "polytope" of the one plane 0 . x + 1 <= 0: cast_hull reports a miss for every ray


def cast_grouped(R, p, tab, o, d, tmax, hulls, spheres):
    """cast() with the hulls' thousands of facets kept away from the rays that cannot meet them: the rays (unit d) are grouped by the set of hulls whose ball their line
    passes within 1 % + 1 mm of, and each group goes through cast() with the other hulls replaced by NO_HULL.  A ray outside a hull's ball misses the hull, so every ray
    gets the answer cast() gives it with all hulls - by cast()'s own arithmetic."""
    keys = sorted(hulls)
    near = np.zeros((len(d), len(keys)), dtype=bool)
    for i, c in enumerate(keys):
        ctr, rad = spheres[c]
        oc = ctr - o
        along = (oc * d).sum(1)
        near[:, i] = np.linalg.norm(oc - d * along[:, None], axis=1) <= 1.01 * rad + 1e-3
    t, who, nrm = np.full(len(d), np.inf), np.full(len(d), -1), np.zeros((len(d), 3))
    groups, inv = np.unique(near, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for g, mask in enumerate(groups):
        sel = inv == g
        t[sel], who[sel], nrm[sel] = cast(R, p, tab, o[sel], d[sel], tmax, {c: (hulls[c] if mask[i] else NO_HULL) for i, c in enumerate(keys)})
    return t, who, nrm


def pixel_rays(eye, target, up, fov, aspect, w, h):
    """eye-to-pixel-centre unit directions [h * w, 3] and the forward axis, float64 (reference_image's arithmetic; moved here from tests/test_gpu_render_layers.py)"""
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(0.5 * np.radians(fov))
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    nx = (2 * (px.ravel() + 0.5) / w - 1) * th * aspect
    ny = (1 - 2 * (py.ravel() + 0.5) / h) * th
    d = f + nx[:, None] * s + ny[:, None] * u
    return d / np.linalg.norm(d, axis=1, keepdims=True), f


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the gripper camera

def quat_matrix(q):
    """getMatrixFromQuaternion: the rotation matrix of a unit quaternion (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def gripper_basis(pos, quat):
    """(forward, right, up) of the reference's gripper camera (environments.py:33-49) for the EE link's pose, its arithmetic line by line in float64: the link's Euler
    angles, (0, -pi / 2, 0) added to them, back to a quaternion and its matrix; the camera vector is that matrix times (1, 0, 0), the up vector that matrix times
    (0, 0, 1); computeViewMatrix(pos, pos + camera vector, up vector) then has f = the camera vector, s = f x up normalised, u = s x f.  The two Euler conversions are
    the oracle's (getEulerFromQuaternion / getQuaternionFromEuler), which tests/test_oracle_golden.py pins to the recorded PyBullet calls and to their identities.

    Worked out, f = Rz(yaw) Ry(pitch) z and u = Rz(yaw) Ry(pitch) (-cos roll, -sin roll, 0): no fixed rotation of the link frame.  It is the link's (-z, +x) only at
    roll = pi, and (+z, -x) at roll = 0."""
    from oracle import euler_from_quat, quat_from_euler
    ori = euler_from_quat(np.asarray(quat, dtype=np.float64)) + np.array([0.0, -PI / 2, 0.0])
    rot = quat_matrix(quat_from_euler(ori))
    cam, up0 = rot @ np.array([1.0, 0.0, 0.0]), rot @ np.array([0.0, 0.0, 1.0])
    f = cam / np.linalg.norm(cam)
    s = np.cross(f, up0)
    s /= np.linalg.norm(s)
    return f, s, np.cross(s, f)


def link_frame_basis(quat):
    """what the library drew until this table existed: forward = -z, up = +x of the link frame"""
    R = quat_matrix(np.asarray(quat, dtype=np.float64))
    f, u = -R[:, 2], R[:, 0]
    return f, np.cross(f, u), u


def basis_angle(a, b):
    """how far camera basis b = (forward, right, up) lies from a, in degrees: the larger of the angles between the two forward axes and between the two up axes"""
    return float(max(np.degrees(np.arccos(np.clip(a[k] @ b[k], -1, 1))) for k in (0, 2)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# states

# The reference's camera looks along Rz(yaw) Ry(pitch) z: upwards by cos(pitch) whatever the roll.  With the hand level it sees the sky and the arm's own wrist (the reset
# pose), so these poses pitch the EE by about a radian and hold it 6 to 22 cm above the table: the camera then looks some 30 degrees above the horizon at the fixtures.
GRIPPER_JOINTS.update({
    ('ur5', 'grip_pi'): [-1.4721, -2.7484, -1.5813, 2.3379, 0.6269, 0.5098],               # roll -3.135, pitch +1.006, yaw +1.966
    ('ur5', 'grip_a'): [-1.6645, -2.6979, -1.3195, -0.0967, -0.4513, 2.0277],              # roll +2.281, pitch +0.985, yaw +0.262
    ('ur5', 'grip_b'): [-2.4067, -1.909, -1.966, -1.4998, 2.7637, 2.0662],                 # roll -0.881, pitch -1.096, yaw -1.230
    ('panda', 'grip_pi'): [-0.7457, 1.1959, 0.8247, -1.9005, 1.126, 1.6519, -0.2948],      # roll -3.115, pitch -1.052, yaw -1.487
    ('panda', 'grip_a'): [0.8813, 0.3635, -0.1803, -2.5626, -2.4343, 1.6245, 2.8555],      # roll -1.845, pitch +0.958, yaw +1.353
    ('panda', 'grip_b'): [0.1276, 0.9941, 0.7698, -1.108, -0.8502, 0.5469, -1.3272]})      # roll -0.959, pitch -1.150, yaw -1.202


def state_layout(o):
    """(arm joints in the chain, first free body, first scene joint) of an oracle's state vector: q [n_arm], qd [n_arm], 13 per free body, scene joints, their rates"""
    n = o.n_arm
    nfree = o.flags()['num_objects'] + 1
    return (7 if n == 9 else 6), 2 * n, 2 * n + 13 * nfree


def build_state(gid, state, env_index=0, f32=True):
    """an oracle of this id in this state.  Every number written is an fp32 value, so the device's float record holds the same."""
    from oracle import OracleEnv
    o = OracleEnv(gid, seed=SEEDS[gid], env_index=env_index, f32=True)
    o.reset()
    if state != 'reset':
        assert gid != W2, 'the wide id is used at its reset state only'
        arm = arm_of(gid)
        chain, free, joint = state_layout(o)
        s = o.get_state()
        if state == 'arm':
            s[:chain] += ARM_DELTA[arm]
            s[chain:o.n_arm] = GRIPPER_HALF[arm]
        elif state == 'scene':
            s[free + 2] += 0.08
            s[free + 3:free + 7] = np.array([0.3, -0.4, 0.5, 0.7]) / np.linalg.norm([0.3, -0.4, 0.5, 0.7])
            s[free + 13 + 1] = -0.06
            s[joint:joint + 3] = [0.12, 0.01, 1.5]
        else:
            s[:chain] = GRIPPER_JOINTS[(arm, state)]
        s[o.n_arm:2 * o.n_arm] = 0.0
        s = s.astype(F32).astype(np.float64)
        o.set_state(s)
    if not f32:          # the fp64 oracle holding the same numbers: what differs is the arithmetic of its forward kinematics
        o64 = OracleEnv(gid, seed=SEEDS[gid], env_index=env_index, f32=False)
        o64.reset()
        o64.set_state(o.get_state())
        return o64
    return o


def block_position(o):
    _, free, _ = state_layout(o)
    return o.get_state()[free:free + 3].astype(F32).astype(np.float64)


def camera_kwargs(name, o):
    """the arguments of VecPlayEnv.camera / camera_rows for a named camera; the cameras aimed at the block take its position from the oracle's state"""
    kw = dict(CAMERAS[name])
    if kw.get('target') == 'edge':
        kw['target'] = (block_position(o) + [0.0, -0.025, 0.025]).tolist()          # the block's upper front edge (10 x 5 x 5 cm) at yaw 90
    elif kw.get('target') == 'block':
        kw['target'] = block_position(o).tolist()
    return kw


def camera_values(cam):
    """dict(eye, target, up, fov, aspect, gripper) in float64 of the float32 numbers the device is given: from an rp_camera structure or from a row of cameras()"""
    if hasattr(cam, 'fov_deg'):
        return dict(eye=np.array(list(cam.eye), dtype=np.float64), target=np.array(list(cam.target), dtype=np.float64), up=np.array(list(cam.up), dtype=np.float64),
                    fov=float(cam.fov_deg), aspect=float(cam.aspect), gripper=cam.mode == 1)
    row = np.asarray(cam, dtype=F32).astype(np.float64)
    assert row.shape == (11,)
    return dict(eye=row[0:3], target=row[3:6], up=row[6:9], fov=float(row[9]), aspect=float(row[10]), gripper=False)


def host_camera(name, o, env_index=0):
    """camera_values of a named camera without a device: the rows camera_rows builds on the host (tests/test_gpu_camera_cases.py holds camera() to them bit for bit)"""
    from roboticsplayroompybullet_amd.vec_env import camera_rows
    if name == 'rows':
        return camera_values(camera_rows(**ROWS)[env_index].numpy())
    kw = camera_kwargs(name, o)
    gripper = kw.pop('gripper', False)
    c = camera_values(camera_rows(**kw)[0].numpy())
    c['gripper'] = gripper
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the reference picture

def collider_colours(o, tab):
    """rgb [n, 3] with the toggles' colours (environments.py:469-483): the globe is red while the button is pressed (q < 0.025), the grill while the dial reads < 0.5"""
    from oracle import dial_to_0_1_range
    _, _, joint = state_layout(o)
    s = o.get_state()
    rgb = tab[:, 4:7].copy()
    for c in range(len(tab)):
        if tab[c, 7] == 1:
            rgb[c] = [1, 0, 0] if s[joint + 1] < 0.025 else [1, 1, 1]
        if tab[c, 7] == 2:
            rgb[c] = [1, 0, 0] if dial_to_0_1_range(s[joint + 2]) < 0.5 else [1, 1, 1]
    return rgb


def ghost_records(o, arm=False):
    """the colliders of an oracle put into a sub-goal's state, as ghosts: (R, p, tab, hulls, hull_spheres, rgb, colliders) of those whose body lies beyond the arm (arm=False: objects,
    drawer, door, button, dial) or on it (arm=True: the Panda's ghost arm)"""
    R, p, tab = o.colliders()
    body = np.array([c['body'] for c in o.collider_list()])
    pick = np.flatnonzero((body >= 1) & (body <= o.n_arm) if arm else body > o.n_arm)
    hulls, spheres = (oracle_hulls(o), hull_spheres(o)) if arm else ({}, {})
    return (R[pick], p[pick], tab[pick], {i: hulls[c] for i, c in enumerate(pick) if c in hulls}, {i: spheres[c] for i, c in enumerate(pick) if c in hulls},
            collider_colours(o, tab)[pick], pick)


def sub_goal_oracle(gid, o, sub_goal, env_index=0):
    """a second oracle in the state a sub-goal vector names (environments.py:606-690): objects' positions and quaternions, the drawer's y, and the three joint values
    written raw as environments.py:695-703 does"""
    from oracle import OracleEnv
    g = OracleEnv(gid, seed=SEEDS[gid], env_index=env_index, f32=True)
    g.reset()
    _, free, joint = state_layout(o)
    s = o.get_state()
    nobj = o.flags()['num_objects']
    sub_goal = np.asarray(sub_goal, dtype=F32).astype(np.float64)
    assert len(sub_goal) == 7 * nobj + 4
    for b in range(nobj):
        s[free + 13 * b:free + 13 * b + 7] = sub_goal[7 * b:7 * b + 7]
    s[free + 13 * nobj + 1] = sub_goal[7 * nobj]
    s[joint:joint + 3] = sub_goal[7 * nobj + 1:7 * nobj + 4]
    g.set_state(s)
    return g


def achieved_goal(o):
    ag = np.array(o.calc_state()['achieved_goal'])
    o.clear_quat_memory()
    return ag.astype(F32).astype(np.float64)


def sub_goal_vector(gid, o, entries):
    """the state's achieved goal with the named GHOST_ENTRIES of the id moved"""
    sg = achieved_goal(o)
    for k in entries:
        i, v, relative = GHOST_ENTRIES[gid][k]
        sg[i] = sg[i] + v if relative else v
    return sg.astype(F32).astype(np.float64)


def ghost_arm_pose(o):
    """[pos3, quat4, gripper] of the ghost arm: the EE pose the observation carries, moved by GHOST_ARM_OFFSET"""
    ee = np.array(o.calc_state()['obs_quat'][0:7])
    o.clear_quat_memory()
    return np.concatenate([ee[0:3] + GHOST_ARM_OFFSET, ee[3:7], [0.0]]).astype(F32).astype(np.float64)


def ghost_arm_oracle(gid, o, pose, env_index=0):
    """a second oracle whose arm stands where the Panda's ghost arm does (environments.py:575-593, 623-637): the rest pose, one IK call of 20 iterations towards the pose
    [pos3, quat4, gripper], joints [0:6] taken"""
    from oracle import OracleEnv
    g = OracleEnv(gid, seed=SEEDS[gid], env_index=env_index, f32=True)
    g.reset()
    g.set_state(o.get_state())
    rest = g.rest_pose()
    pose = np.asarray(pose, dtype=F32).astype(np.float64)
    sol = g.ik(pose[0:3], pose[3:7], rest, max_iter=20)
    q = rest.copy()
    q[:6] = sol[:6]
    g.set_arm_q(q)
    return g


def camera_basis(o, cam):
    """(eye, target, up) the rays start from: the camera's own, or for the gripper camera the reference's basis at the oracle's EE link (cam['basis'] == 'link': the
    link-frame basis instead, to show that the two pictures differ)"""
    if not cam['gripper']:
        return cam['eye'], cam['target'], cam['up']
    pos, quat, _, _ = o.site_pose(0)
    f, _, u = link_frame_basis(quat) if cam.get('basis') == 'link' else gripper_basis(pos, quat)
    return pos, pos + f, u


def reference_layers(o, cam, w, h, near=NEAR, far=FAR, ghosts=None, poses=None):
    """the three layers of one env in float64 from the oracle's colliders: dict(rgb [h, w, 3] in [0, 1] before rounding, z [h, w] eye-space depth in metres (far on a
    miss), seg [h, w] = collider | (link + 1) << 24 (-1 on a miss)) and, for the tests' own use, who [h, w] the collider, ndotd [h, w] = |n . d| at the hit (1 on a miss)
    and tint [h, w] = where a ghost was blended in.  cam: camera_values.  ghosts: a list of ghost_records; by the rule in the header of rp_render.cuh the nearest ghost hit
    nearer than the nearest solid hit - a solid miss counts as t = 10 - blends 0.5 colour + 0.5 shade(ghost); ghosts never touch z or seg.  poses: another oracle whose
    collider poses are cast instead (the spread of the reference itself), the rays staying o's.  near is unused by the metres depth and kept for the call's symmetry."""
    eye, target, up = camera_basis(o, cam)
    d, f = pixel_rays(eye, target, up, cam['fov'], cam['aspect'], w, h)
    src = poses if poses is not None else o
    R, p, tab = src.colliders()
    org = np.tile(eye, (len(d), 1))
    t, who, nrm = cast_grouped(R, p, tab, org, d, 10.0, oracle_hulls(src), hull_spheres(src))
    hit = who >= 0
    safe = np.maximum(who, 0)
    shade = 0.45 + 0.55 * np.maximum(0, nrm @ LIGHT)
    col = np.where(hit[:, None], collider_colours(src, tab)[safe] * shade[:, None], BACKGROUND)
    tint = np.zeros(len(d), dtype=bool)
    if ghosts:
        gt, gcol = np.full(len(d), 10.0), np.zeros((len(d), 3))
        for gR, gp, gtab, ghulls, gspheres, grgb, _ in ghosts:
            t2, who2, nrm2 = cast_grouped(gR, gp, gtab, org, d, 10.0, ghulls, gspheres)
            k2 = 0.45 + 0.55 * np.maximum(0, nrm2 @ LIGHT)
            nearer = (who2 >= 0) & (t2 < gt)
            gt = np.where(nearer, t2, gt)
            gcol = np.where(nearer[:, None], grgb[np.maximum(who2, 0)] * k2[:, None], gcol)
        tint = gt < np.where(hit, t, 10.0)
        col = np.where(tint[:, None], 0.5 * col + 0.5 * gcol, col)
    seg = np.where(hit, safe | ((tab[safe, 8].astype(int) + 1) << 24), -1)
    z = np.where(hit, np.where(hit, t, 0.0) * (d @ f), far)
    ndotd = np.where(hit, np.abs((nrm * d).sum(1)), 1.0)
    sh = (h, w)
    return dict(rgb=np.clip(col, 0, 1).reshape(h, w, 3), z=z.reshape(sh), seg=seg.reshape(sh), who=who.reshape(sh), ndotd=ndotd.reshape(sh), tint=tint.reshape(sh))


def to_bytes(rgb):
    """the image's rounding: floor(255 c + 0.5)"""
    return np.floor(rgb * 255 + 0.5).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the table

def cases():
    """every (id, state, camera, (w, h), env) of the layer and gripper checks"""
    out = []
    for gid in IDS:
        for state in STATES[gid]:
            for name in CAMERA_NAMES:
                for size in SIZES:
                    for e in (range(NUM_ENVS) if name == 'rows' or gid == W2 else (0,)):
                        out.append((gid, state, name, size, e))
    for gid in (U, V):
        for state in GRIPPER_STATES:
            if state != 'reset':
                out.append((gid, state, 'gripper', SIZES[0], 0))
        if gid == U:
            out += [(gid, state, 'gripper', GRIPPER_SIZE_UR5, 0) for state in GRIPPER_STATES]
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(gid, state, env_index=0, f32=True):
    return build_state(gid, state, env_index if gid == W2 else 0, f32)


def measure(case):
    """what the CPU test asserts of a case: dict(spread, graze, hits, colliders) and for a gripper case euler and off (degrees between the two bases)"""
    from oracle import euler_from_quat
    gid, state, name, (w, h), e = case
    o, o64 = oracle_of(gid, state, e), oracle_of(gid, state, e, False)
    cam = host_camera(name, o, e)
    a, b = reference_layers(o, cam, w, h), reference_layers(o, cam, w, h, poses=o64)
    out = dict(spread=float(((a['seg'] != b['seg']) | (b['ndotd'] < GRAZE)).mean()), differ=int((a['seg'] != b['seg']).sum()), graze=int((b['ndotd'] < GRAZE).sum()),
               hits=float((a['who'] >= 0).mean()), colliders=len(np.unique(a['who'][a['who'] >= 0])))
    if name == 'gripper':
        pos, quat, _, _ = o.site_pose(0)
        out['euler'] = euler_from_quat(quat)
        out['off'] = basis_angle(gripper_basis(pos, quat), link_frame_basis(quat))
    return out


def main():
    print('# python tests/camera_cases.py: id state camera width x height env | share of pixels the fp32 and fp64 oracle disagree on or the fp64 cast grazes (cap %g) = '
          'differing + grazing pixels | hit share | colliders in view | gripper: EE Euler angles, degrees between the link-frame basis (-z, +x) and the reference\'s' % SPREAD_CAP)
    for case in cases():
        gid, state, name, (w, h), e = case
        m = measure(case)
        line = '%-24s %-8s %-8s %3d x %3d env %d | spread %.5f = %d + %d px | hits %.3f | colliders %2d' % (gid, state, name, w, h, e, m['spread'], m['differ'], m['graze'],
                                                                                                          m['hits'], m['colliders'])
        if 'euler' in m:
            line += ' | roll %+.4f pitch %+.4f yaw %+.4f, off %.2f deg' % (*m['euler'], m['off'])
        print(line)


if __name__ == '__main__':
    main()
