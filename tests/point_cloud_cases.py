"""The point-cloud rule of rp_render_points / rp_set_image_points (include/rp_playroom.h) in numpy, shared by tests/test_point_cloud_rule.py (CPU: the rule on synthetic
layers) and tests/test_gpu_points.py (the device's selection against it, exactly; its coordinates against the float64 formula below).

For one env and one view of width x height, depth in metres and the packed segmentation as render_layers writes them:
  pixels in row-major order i = y * width + x; pixel i is VALID iff seg[i] != -1, bit (seg[i] & 0xFF) of drop is clear and (max_depth <= 0 or depth[i] <= max_depth);
  n = the valid pixels, r(i) = the rank of a valid pixel among them, P = max_points.
  n <= P: slot r(i) takes pixel i, slots n .. P - 1 are padding (xyz 0, seg -1, rgb 0).
  n >  P: slot j takes the valid pixel of rank floor(j * n / P) (64-bit integers).
  count = n, not capped.
Nothing here knows the device: the selection is index arithmetic on the layers it is handed."""
import numpy as np

F32 = np.float32
MAX_COL = 64          # RP_MAX_COL: the width of the drop mask


def drop_mask(colliders):
    """the uint64 whose bit c is set for every collider index c of the iterable"""
    m = 0
    for c in colliders:
        c = int(c)
        assert 0 <= c < MAX_COL, c
        m |= 1 << c
    return m


def valid_pixels(depth, seg, max_depth=0.0, drop=0):
    """bool [height * width] in scan order.  depth is compared as the float32 it is, max_depth as the float32 the spec carries"""
    depth = np.asarray(depth, dtype=F32).ravel()
    seg = np.asarray(seg, dtype=np.int32).ravel()
    lut = np.array([c < MAX_COL and (int(drop) >> c) & 1 == 1 for c in range(256)], dtype=bool)          # by the low byte: bits beyond MAX_COL do not exist
    ok = (seg != -1) & ~lut[seg & 0xFF]
    md = F32(max_depth)
    if md > 0:
        ok &= depth <= md
    return ok


def selected_ranks(n, P):
    """the rank that each slot j < min(n, P) takes, int64 [min(n, P)]: j itself when n <= P, floor(j * n / P) when n > P (Python integers: no width to overflow)"""
    n, P = int(n), int(P)
    if n <= P:
        return np.arange(n, dtype=np.int64)
    return np.array([(j * n) // P for j in range(P)], dtype=np.int64)


def local_decision(r, n, P):
    """what the device's thread of rank r decides alone when n > P: (taken, slot) with slot j0 = ceil(r * P / n), taken iff j0 < P and floor(j0 * n / P) == r"""
    r, n, P = int(r), int(n), int(P)
    j0 = -((-r * P) // n)
    return (j0 < P and (j0 * n) // P == r), j0


def select(depth, seg, P, max_depth=0.0, drop=0):
    """(pixel [P] int64: the scan index each slot takes, -1 for padding; n)"""
    ok = valid_pixels(depth, seg, max_depth, drop)
    hits = np.flatnonzero(ok)
    n = len(hits)
    pix = np.full(int(P), -1, dtype=np.int64)
    ranks = selected_ranks(n, P)
    pix[:len(ranks)] = hits[ranks]
    return pix, n


def cloud(depth, seg, P, max_depth=0.0, drop=0, rgb=None):
    """dict(pixel [P], segmentation [P] int32, count, rgb [P, 3] uint8 if rgb is given) of one env by the rule; padding: segmentation -1, rgb 0"""
    pix, n = select(depth, seg, P, max_depth, drop)
    seg = np.asarray(seg, dtype=np.int32).ravel()
    real = pix >= 0
    out = dict(pixel=pix, count=n, segmentation=np.where(real, seg[np.maximum(pix, 0)], -1).astype(np.int32))
    if rgb is not None:
        flat = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
        out['rgb'] = np.where(real[:, None], flat[np.maximum(pix, 0)], 0).astype(np.uint8)
    return out


def pixel_scale(pix, width, height, fov, aspect):
    """(nx, ny) float64 of scan indices: camera_cases.pixel_rays' expressions, the tangent taken in float64 of the float32 field of view"""
    pix = np.asarray(pix, dtype=np.int64)
    y, x = pix // width, pix % width
    th = np.tan(0.5 * np.radians(float(fov)))
    return (2 * (x + 0.5) / width - 1) * th * aspect, (1 - 2 * (y + 0.5) / height) * th


def xyz_camera(pix, z, width, height, fov, aspect):
    """float64 [k, 3] = (nx z, ny z, z) along (right, up, forward)"""
    nx, ny = pixel_scale(pix, width, height, fov, aspect)
    z = np.asarray(z, dtype=np.float64)
    return np.stack([nx * z, ny * z, z], axis=1)


def basis(eye, target, up):
    """(eye, forward, right, up) float64 as camera_cases.pixel_rays builds them"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    return eye, f, s, np.cross(s, f)


def xyz_world(pix, z, width, height, fov, aspect, eye, target, up):
    """float64 [k, 3] = eye + (forward + right nx + up ny) z"""
    nx, ny = pixel_scale(pix, width, height, fov, aspect)
    e, f, s, u = basis(eye, target, up)
    z = np.asarray(z, dtype=np.float64)
    return e + (f + nx[:, None] * s + ny[:, None] * u) * z[:, None]


def camera_to_world(xyz_cam, eye, target, up):
    """camera-frame points (right, up, forward) mapped through a basis: eye + right x + up y + forward z, float64"""
    e, f, s, u = basis(eye, target, up)
    p = np.asarray(xyz_cam, dtype=np.float64)
    return e + p[:, 0:1] * s + p[:, 1:2] * u + p[:, 2:3] * f
