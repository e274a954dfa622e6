"""The point-cloud rule's numpy reference (tests/point_cloud_cases.py) on synthetic layers, without a device: which ranks n > P selects, the boundaries n == P,
n == P + 1, n == 0 and P == 1, the drop and max_depth filters, the padding values, and one case whose products r * P pass 2^32, against Python's big integers."""
import numpy as np
import pytest

import point_cloud_cases as pc


def layers(width, height, seed, miss=0.3, colliders=(0, 3, 7, 12, 40, 63)):
    """a depth / segmentation / rgb triple in render_layers' formats: misses read -1 and 10 m, hits a collider of `colliders` with link + 1 in the top byte"""
    rng = np.random.default_rng(seed)
    npix = width * height
    col = rng.choice(colliders, npix)
    link = rng.integers(-1, 9, npix)
    hit = rng.random(npix) >= miss
    seg = np.where(hit, col | ((link + 1) << 24), -1).astype(np.int32)
    depth = np.where(hit, rng.uniform(0.2, 3.0, npix), 10.0).astype(np.float32)
    rgb = rng.integers(0, 256, (npix, 3)).astype(np.uint8)
    return depth.reshape(height, width), seg.reshape(height, width), rgb.reshape(height, width, 3)


@pytest.mark.parametrize('n,P', ((7, 3), (100, 99), (1000, 7), (257, 256), (7056, 1024), (90000, 65536), (5, 4)))
def test_subsampling_selects_floor_j_n_over_p(n, P):
    """n > P: slot j takes rank floor(j n / P) exactly; the ranks rise strictly, the first is 0, the last is below n; and the local decision of every rank - the one
    the device's threads make - names exactly those slots"""
    ranks = pc.selected_ranks(n, P)
    assert ranks.dtype == np.int64 and len(ranks) == P
    assert [int(r) for r in ranks] == [(j * n) // P for j in range(P)]
    assert ranks[0] == 0 and ranks[-1] < n and (np.diff(ranks) > 0).all()
    taken = {}
    for r in range(n):
        ok, j0 = pc.local_decision(r, n, P)
        if ok:
            assert j0 not in taken
            taken[j0] = r
    assert sorted(taken) == list(range(P)) and [taken[j] for j in range(P)] == [int(r) for r in ranks]


def test_boundaries_n_equal_p_one_more_none_and_one_slot():
    depth, seg, rgb = layers(17, 16, 1)
    n = int((seg != -1).sum())
    hits = np.flatnonzero(seg.ravel() != -1)
    assert 100 < n < 272
    # n == P: every hit, in scan order, no padding
    c = pc.cloud(depth, seg, n, rgb=rgb)
    assert c['count'] == n and (c['pixel'] == hits).all() and (c['segmentation'] == seg.ravel()[hits]).all() and (c['rgb'] == rgb.reshape(-1, 3)[hits]).all()
    # n == P + 1: exactly one hit is left out, and it is not the first
    c = pc.cloud(depth, seg, n - 1)
    assert c['count'] == n and len(set(c['pixel'])) == n - 1 and set(c['pixel']) < set(hits) and c['pixel'][0] == hits[0]
    assert (c['pixel'] == hits[[(j * n) // (n - 1) for j in range(n - 1)]]).all()
    # n == P - 1: one padding slot
    c = pc.cloud(depth, seg, n + 1, rgb=rgb)
    assert (c['pixel'][:n] == hits).all() and c['pixel'][n] == -1 and c['segmentation'][n] == -1 and (c['rgb'][n] == 0).all()
    # P == 1: the first hit, whatever n
    c = pc.cloud(depth, seg, 1)
    assert c['count'] == n and c['pixel'].tolist() == [hits[0]]
    # n == 0: padding alone
    none = np.full_like(seg, -1)
    c = pc.cloud(np.full_like(depth, 10.0), none, 5, rgb=rgb)
    assert c['count'] == 0 and (c['pixel'] == -1).all() and (c['segmentation'] == -1).all() and (c['rgb'] == 0).all()
    # P beyond the image: every hit, then padding
    c = pc.cloud(depth, seg, 300)
    assert c['count'] == n and (c['pixel'][:n] == hits).all() and (c['pixel'][n:] == -1).all()


def test_the_filters_drop_colliders_and_cut_the_depth():
    depth, seg, _ = layers(70, 45, 2)
    flat, z = seg.ravel(), depth.ravel()
    hit = flat != -1
    # drop: by the LOW BYTE of the packed value, whatever the link byte says
    drop = pc.drop_mask((3, 63))
    ok = pc.valid_pixels(depth, seg, drop=drop)
    want = hit & ~np.isin(flat & 0xFF, (3, 63))
    assert (ok == want).all() and 0 < want.sum() < hit.sum()
    assert pc.drop_mask(()) == 0 and pc.drop_mask((0,)) == 1 and pc.drop_mask((63,)) == 1 << 63
    # max_depth: <= keeps the boundary value; 0 and negatives mean no limit; the comparison is float32's
    cut = float(np.sort(z[hit])[hit.sum() // 2])
    ok = pc.valid_pixels(depth, seg, max_depth=cut)
    assert (ok == (hit & (z <= np.float32(cut)))).all() and ok[np.flatnonzero(hit & (z == np.float32(cut)))].all() and 0 < ok.sum() < hit.sum()
    for no_limit in (0.0, -1.0):
        assert (pc.valid_pixels(depth, seg, max_depth=no_limit) == hit).all()
    # both at once, and a miss is never valid even at a depth inside the limit
    ok = pc.valid_pixels(depth, seg, max_depth=cut, drop=drop)
    assert (ok == (want & (z <= np.float32(cut)))).all()
    assert not pc.valid_pixels(np.float32([[1.0]]), np.int32([[-1]]), max_depth=5.0).any()
    pix, n = pc.select(depth, seg, 64, max_depth=cut, drop=drop)
    assert n == ok.sum() > 64 and ok[pix].all() and (np.diff(pix) > 0).all()


def test_padding_values_and_coordinates_of_a_known_pixel():
    depth, seg, rgb = layers(15, 17, 3, miss=0.9)
    c = pc.cloud(depth, seg, 255, rgb=rgb)
    n = c['count']
    assert 0 < n < 255
    assert (c['pixel'][n:] == -1).all() and (c['segmentation'][n:] == -1).all() and (c['rgb'][n:] == 0).all() and c['rgb'].dtype == np.uint8
    assert (c['segmentation'][:n] != -1).all()
    # the centre pixel of an odd image looks straight ahead: (0, 0, z) in the camera frame, eye + forward z in the world frame
    w = h = 5
    centre = np.array([2 * w + 2])
    cam = pc.xyz_camera(centre, [2.0], w, h, 50.0, 1.3)
    assert np.allclose(cam, [[0.0, 0.0, 2.0]], atol=1e-15)
    eye, target, up = np.array([1.0, -2.0, 0.5]), np.array([1.0, 0.0, 0.5]), np.array([0.0, 0.0, 1.0])
    assert np.allclose(pc.xyz_world(centre, [2.0], w, h, 50.0, 1.3, eye, target, up), [[1.0, 0.0, 0.5]], atol=1e-15)
    # the top-left pixel: right is +x here, up is +z; both formulas agree through camera_to_world
    corner = np.array([0])
    cam = pc.xyz_camera(corner, [1.5], w, h, 90.0, 2.0)
    assert np.allclose(cam, [[-0.8 * 2.0 * 1.5, 0.8 * 1.5, 1.5]], atol=1e-12)
    assert np.allclose(pc.camera_to_world(cam, eye, target, up), pc.xyz_world(corner, [1.5], w, h, 90.0, 2.0, eye, target, up), atol=1e-12)


def test_products_beyond_32_bits_against_python_integers():
    """n = 90000 hits, P = 65536: r * P reaches 5.9e9 > 2^32.  The reference is held to Python's integers, and so is the 32-bit mistake it must not make"""
    n, P = 90000, 65536
    assert (n - 1) * P > 2 ** 32
    ranks = pc.selected_ranks(n, P)
    for j in (0, 1, 47721, 47722, 65535):
        assert int(ranks[j]) == (j * n) // P
    assert 47722 * n > 2 ** 32 > 47721 * n          # the first slot whose product j * n passes 2^32 ...
    wrapped = ((47722 * n) % 2 ** 32) // P
    assert wrapped != int(ranks[47722])             # ... and what 32-bit arithmetic would have picked there
    for r in (0, 65536, 65537, 89999, 89998, 2 ** 16 + 12345):
        ok, j0 = pc.local_decision(r, n, P)
        assert j0 == -((-r * P) // n) and ok == (j0 < P and int(ranks[min(j0, P - 1)]) == r)
    depth = np.full((300, 300), 1.0, dtype=np.float32)
    seg = np.zeros((300, 300), dtype=np.int32)
    pix, count = pc.select(depth, seg, P)
    assert count == n and (pix == ranks).all()
