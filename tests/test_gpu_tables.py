"""The one set / get path behind the dynamics, wrench and actuation tables (k_set_table / k_get_table), at the shapes where a kernel shared by all three can go wrong
and the per-table tests (N = 6 or 8: one 256-thread block) cannot see it: tables of several blocks with a ragged last one (N = 300: 6000 to 30600 entries, never a
multiple of 256), a zero-width column block (UR5Reach-v0 has no free body: its mass block) and the wide build.  Run with -m gpu on the MI355X box.

No env is stepped or reset.  A torch model of the table starts from get_*(); for every non-empty subset of the column blocks, rows 1 and N and every mask (none; one
that treats env 0 and env N - 1 differently; all zero) the setter gets fresh random device tensors and get_*() must equal the torch.where model bit for bit.  Then the
raw getter is called with each single block and NULL for the others into sentinel-filled buffers: that block exact, the sentinel untouched around it.
"""
import ctypes as C
import itertools

import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

IDS = ('UR5PlayAbsRPY1Obj-v0', 'UR5Reach-v0', 'pandaPlay-v0')      # the headline id; n_free = 0; the wide build
BLOCKS = {'dynamics': ('friction', 'mass'), 'wrench': ('wrench',), 'actuation': ('gravity', 'motor_gain', 'motor_strength')}
SENTINEL, PAD = -12345.0, 256


def bits(t):
    return t.contiguous().view(torch.int32)


def read(env, table):
    """the table as {block: [N, ...]}"""
    got = getattr(env, 'get_' + table)()
    return {'wrench': got} if table == 'wrench' else got


def masks(n, dev):
    m = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)
    m[0], m[n - 1] = 1, 0
    return (None, m, torch.zeros(n, dtype=torch.uint8, device=dev))


def expect(model, src, rows, mask):
    """what a set of `src` ([...] with rows 1, [N, ...] with rows N) under `mask` leaves of the block `model`"""
    new = src if rows != 1 else src[None].expand_as(model)
    if mask is None:
        return new.clone()
    return torch.where(mask.bool().reshape((-1,) + (1,) * (model.dim() - 1)), new, model)


@pytest.mark.parametrize('n', (5, 300))
@pytest.mark.parametrize('gid', IDS)
@pytest.mark.parametrize('table', tuple(BLOCKS))
def test_shared_table_path(table, gid, n):
    from roboticsplayroompybullet_amd import VecPlayEnv
    env = VecPlayEnv(gid, n, seed=1)
    dev, names = env.device, BLOCKS[table]
    setter = getattr(env, 'set_' + table)
    model = read(env, table)
    entries = sum(v[0].numel() for v in model.values()) * n
    if n == 300:
        assert entries > 256 and entries % 256 != 0, entries      # several blocks, the last one ragged
    if gid == 'UR5Reach-v0' and table == 'dynamics':
        assert model['mass'].shape == (n, 0)                      # the zero-width block
    gen = torch.Generator(device=dev).manual_seed(n)

    # every non-empty subset of the blocks x rows x mask (a subset of zero-width blocks alone is all-NULL to the library, which refuses it: not a set)
    for k in range(1, len(names) + 1):
        for subset in itertools.combinations(names, k):
            if not any(model[b][0].numel() for b in subset):
                continue
            for rows, mask in itertools.product((1, n), masks(n, dev)):
                src = {b: 0.25 + torch.rand(model[b].shape[1:] if rows == 1 else model[b].shape, generator=gen, device=dev) for b in subset}
                setter(src['wrench'], mask=mask) if table == 'wrench' else setter(mask=mask, **src)
                for b in subset:
                    model[b] = expect(model[b], src[b], rows, mask)
                got = read(env, table)
                for b in names:
                    assert torch.equal(bits(got[b]), bits(model[b])), (subset, rows, mask is not None and int(mask.sum()), b)

    # one call whose arguments disagree on rows (the first block one row and the others N, and the reverse): the single rows reach every env, the others their own
    live = [b for b in names if model[b][0].numel()]
    for single in ((live[:1], live[1:]) if len(live) > 1 else ()):
        src = {b: 0.25 + torch.rand(model[b].shape[1:] if b in single else model[b].shape, generator=gen, device=dev) for b in live}
        setter(**src)
        for b in live:
            model[b] = expect(model[b], src[b], 1 if b in single else n, None)
        got = read(env, table)
        for b in names:
            assert torch.equal(bits(got[b]), bits(model[b])), (single, b)

    # the wrench table's NULL source: zeros in exactly the masked envs
    if table == 'wrench':
        for mask in masks(n, dev):
            full = 0.25 + torch.rand(model['wrench'].shape, generator=gen, device=dev)
            env.set_wrench(full)
            env.set_wrench(None, mask=mask)
            model['wrench'] = expect(full, torch.zeros_like(full), n, mask)
            assert torch.equal(bits(env.get_wrench()), bits(model['wrench'])), mask is not None and int(mask.sum())

    # the raw getter, one block at a time into a sentinel-filled buffer, NULL for the others
    raw = getattr(env.lib, 'rp_get_' + table)
    for i, b in enumerate(names):
        buf = torch.full((model[b].numel() + 2 * PAD,), SENTINEL, device=dev)
        ptrs = [None] * len(names)
        ptrs[i] = C.c_void_p(buf.data_ptr() + 4 * PAD)
        assert raw(env.h, *ptrs, env._stream()) == 0, (b, env.lib.rp_last_error(env.h))
        assert torch.equal(bits(buf[PAD:PAD + model[b].numel()]), bits(model[b].reshape(-1))), b
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + model[b].numel():] == SENTINEL).all()), b
    torch.cuda.synchronize()
    env.close()
