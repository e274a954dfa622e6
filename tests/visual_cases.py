"""The float64 reference of the per-env visuals (rp_set_visuals), shared by tests/test_visuals_abi.py (CPU: the reference against camera_cases' own) and
tests/test_gpu_visuals.py (the device against it).

reference_rgb is camera_cases.reference_layers' colour layer with the three constants it draws from - the collider table's rgb, LIGHT with 0.45 / 0.55, BACKGROUND - taken
from the arguments instead: the same rays (pixel_rays over camera_basis), the same cast (cast_grouped over oracle_hulls / hull_spheres), the same toggle colours
(collider_colours' rule, on top of whatever the table says: the globe and the grill show state) and the same ghost rule (ghost_records; the nearest ghost nearer than the
solid hit - a solid miss counts as 10 m - blends half and half).  Its operations stand in reference_layers' order, so with DEFAULT_LIGHT, DEFAULT_BACKGROUND and the table's
own colours the two agree in every bit."""
import numpy as np

import camera_cases as cc

F32 = np.float32
DEFAULT_LIGHT = np.concatenate([cc.LIGHT, [0.45, 0.55]])            # camera_cases' float64 constants: what reference_layers draws with
DEFAULT_BACKGROUND = cc.BACKGROUND.copy()
# the library's float32 defaults (rp_render.cuh's literals), as get_visuals returns them on a fresh handle
DEVICE_LIGHT = np.array([0.2672612, -0.5345225, 0.8017837, 0.45, 0.55], dtype=F32)
DEVICE_BACKGROUND = np.array([0.82, 0.88, 0.96], dtype=F32)


def table_colours(o):
    """the oracle collider table's rgb [n_col, 3]: the default colour part"""
    return o.colliders()[2][:, 4:7].copy()


def toggle_colliders(o):
    """the colliders whose colour shows state (the button's globe, the dial's grill)"""
    return np.flatnonzero(np.isin(o.colliders()[2][:, 7], (1, 2)))


def with_toggles(shown, tab, colour):
    """colour [n, 3] with the rows of the toggle colliders of tab replaced by `shown`'s (collider_colours' red / white for the state of the oracle it was asked about)"""
    out = np.array(colour, dtype=np.float64)
    tog = np.isin(tab[:, 7], (1, 2))
    out[tog] = shown[tog]
    return out


def reference_rgb(o, cam, w, h, colour, light, background, ghosts=None):
    """the colour layer of one env in float64 from the oracle's colliders and this env's visuals row: dict(rgb [h, w, 3] in [0, 1] before rounding, who [h, w] the
    collider hit (-1 on a miss), seg [h, w] = collider | (link + 1) << 24 (-1 on a miss), tint [h, w] = where a ghost was blended in, ghost [h, w] = the collider of
    that ghost (-1 elsewhere)).  colour [n_col, 3], light [5] = direction (used as it stands), ambient, diffuse, background [3]: the float32 values the device was given,
    upcast.  cam: camera_values.  ghosts: a list of camera_cases.ghost_records; a ghost has its collider's colour of the same row."""
    colour, light, background = (np.asarray(v).astype(np.float64) for v in (colour, light, background))
    direction, ambient, diffuse = light[:3].copy(), light[3], light[4]
    eye, target, up = cc.camera_basis(o, cam)
    d, f = cc.pixel_rays(eye, target, up, cam['fov'], cam['aspect'], w, h)
    R, p, tab = o.colliders()
    org = np.tile(eye, (len(d), 1))
    t, who, nrm = cc.cast_grouped(R, p, tab, org, d, 10.0, cc.oracle_hulls(o), cc.hull_spheres(o))
    hit = who >= 0
    safe = np.maximum(who, 0)
    shade = ambient + diffuse * np.maximum(0, nrm @ direction)
    col = np.where(hit[:, None], with_toggles(cc.collider_colours(o, tab), tab, colour)[safe] * shade[:, None], background)
    tint = np.zeros(len(d), dtype=bool)
    gwho = np.full(len(d), -1)
    if ghosts:
        gt, gcol = np.full(len(d), 10.0), np.zeros((len(d), 3))
        for gR, gp, gtab, ghulls, gspheres, grgb, pick in ghosts:
            t2, who2, nrm2 = cc.cast_grouped(gR, gp, gtab, org, d, 10.0, ghulls, gspheres)
            k2 = ambient + diffuse * np.maximum(0, nrm2 @ direction)
            nearer = (who2 >= 0) & (t2 < gt)
            gt = np.where(nearer, t2, gt)
            gcol = np.where(nearer[:, None], with_toggles(grgb, gtab, colour[pick])[np.maximum(who2, 0)] * k2[:, None], gcol)
            gwho = np.where(nearer, pick[np.maximum(who2, 0)], gwho)
        tint = gt < np.where(hit, t, 10.0)
        col = np.where(tint[:, None], 0.5 * col + 0.5 * gcol, col)
        gwho = np.where(tint, gwho, -1)
    seg = np.where(hit, safe | ((tab[safe, 8].astype(int) + 1) << 24), -1)
    sh = (h, w)
    return dict(rgb=np.clip(col, 0, 1).reshape(h, w, 3), who=who.reshape(sh), seg=seg.reshape(sh), tint=tint.reshape(sh), ghost=gwho.reshape(sh))


def random_visuals(n, n_col, seed):
    """n rows that differ in every part, float32: dict(colour [n, n_col, 3] uniform in [0, 1), light [n, 5], background [n, 3]).  Row 0's light comes from below,
    (0, 0, -1); row 1's direction is NOT of unit length (the library uses it as it stands); row 2 has ambient 0.7 and diffuse 0.6, which saturate bright colours and
    exercise the clamp.  Rows beyond 2 repeat the three lights."""
    rng = np.random.default_rng(seed)
    colour = rng.random((n, n_col, 3), dtype=F32)
    lights = np.array([[0.0, 0.0, -1.0, 0.3, 0.7], [0.9, 0.5, 1.4, 0.25, 0.5], [-0.48, 0.6, 0.64, 0.7, 0.6]], dtype=F32)
    light = lights[np.arange(n) % 3]
    background = np.array([[0.1, 0.2, 0.3], [0.95, 0.9, 0.4], [0.5, 0.0, 1.0]], dtype=F32)[np.arange(n) % 3] * (1.0 - 0.1 * (np.arange(n) // 3)[:, None]).astype(F32)
    return dict(colour=colour, light=light.copy(), background=background.astype(F32))
