"""rp_step_autoreset / VecPlayEnv(autoreset=True): the envs that end inside a step reset on the device.  Run with -m gpu on the MI355X box.

The yardstick is the host-driven path the library already has: a twin handle with the same seed that runs rp_step, keeps the rows, and then
rp_reset(mask) with the envs that should have ended.  The counter-keyed RNG makes a reset's draws independent of which other envs reset with it,
so the two must agree bit for bit.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from reset_draws import DRAWS, RNG_COL, decode

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

IDS = ('UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'UR5Reach-v0', 'pandaPlay-v0')
OBS = ('obs_quat', 'achieved_goal', 'desired_goal', 'controllable_achieved_goal', 'full_positional_state', 'joints', 'velocity', 'observation',
       'gripper_proprioception')
LO = np.array([-0.18, 0.0, 0.05, -0.5, -0.5, -0.5, -1.0])
HI = np.array([0.18, 0.3, 0.3, 0.5, 0.5, 0.5, 1.0])


def actions(env, steps, seed):
    """fixed random actions [steps, N, action] on the env's device: workspace targets for the absolute_rpy ids, near-identity poses for absolute_quat"""
    rng = np.random.default_rng(seed)
    n = env.num_envs
    if env.action_type == 'absolute_quat':
        a = np.zeros((steps, n, 8))
        a[..., 0:3] = LO[:3] + (HI[:3] - LO[:3]) * rng.random((steps, n, 3))
        a[..., 3:7] = np.array([0, 0, 0, 1.0]) + 0.2 * (rng.random((steps, n, 4)) - 0.5)
        a[..., 7] = 2 * rng.random((steps, n)) - 1
    else:
        a = LO + (HI - LO) * rng.random((steps, n, 7))
        if not env.env_id.startswith('UR5Play'):
            a[..., 0:3] = np.array([-0.18, -0.18, 0.0]) + np.array([0.36, 0.36, 0.2]) * rng.random((steps, n, 3))
    return torch.tensor(a, dtype=torch.float32, device=env.device)


def end_masks(n, steps, seed, device, p=0.05):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) < p).to(device=device, dtype=torch.uint8) for _ in range(steps)]


def make(gid, n, seed, **kw):
    from roboticsplayroompybullet_amd import VecPlayEnv
    return VecPlayEnv(gid, n, seed=seed, **kw)


def compare_with_twin(A, B, steps, seed, stagger, full_ends=()):
    """A: rp_step_autoreset (time limit = stagger, counters staggered e % stagger, a random 5 % end_mask - all ones in the steps `full_ends` - and the fault
    rule); twin B: rp_step, rows kept, rp_reset(mask of the envs that ended).  A's observations, the pack's observation part and every state row (record +
    contact cache) equal B's after its reset; A's reward / is_success / target_poses and the pack's last two columns equal B's step rows; A's status = B's
    step status | its reset status; terminal_observation = B's step rows; done = the expected mask; the counters follow.  Returns the ends of every step
    and the RNG draws (ST_RNG after - before B's reset) of every env that ended; an env that did not end drew nothing."""
    n = A.num_envs
    dev = A.device
    e = torch.arange(n, device=dev, dtype=torch.int32)
    A.episode_steps = e % stagger
    cnt = (e % stagger).clone()
    acts = actions(A, steps, seed)
    masks = end_masks(n, steps, seed + 1, dev)
    for t in full_ends:
        masks[t] = torch.ones(n, device=dev, dtype=torch.uint8)
    no, na = A.dims['obs_quat'], A.dims['achieved_goal']
    col = RNG_COL[A.wide]
    ends, draws = [], []
    for t in range(steps):
        oa, ra, da, ia = A.step(acts[t], end_mask=masks[t])
        B.step(acts[t])
        kept = {k: B.buf[k].clone() for k in OBS + ('reward', 'is_success', 'target_poses', 'status')}
        kept_pack = B.pack.clone()
        rng0 = B.get_state()[:, col].contiguous().view(torch.int32)
        c1 = cnt + 1
        reason = (c1 >= stagger).int() | (masks[t] != 0).int() * 2 | ((kept['status'] & 3) != 0).int() * 4
        mask = reason != 0
        cnt = torch.where(mask, torch.zeros_like(c1), c1)
        if bool(mask.any()):
            B.reset(mask=mask)
        torch.cuda.synchronize()
        ends.append(int(mask.sum()))
        assert torch.equal(da, mask), t
        assert torch.equal(ia['done_reason'], reason), t
        assert torch.equal(ia['TimeLimit.truncated'], reason == 1), t
        for k in OBS:
            assert torch.equal(oa[k], B.buf[k]), (t, k)
        assert torch.equal(A.pack[:, :no + na], B.pack[:, :no + na]), t
        assert torch.equal(A.pack[:, no + na:], kept_pack[:, no + na:]), t
        assert torch.equal(ra, kept['reward']), t
        assert torch.equal(ia['is_success'], kept['is_success']), t
        assert torch.equal(ia['target_poses'], kept['target_poses']), t
        assert torch.equal(ia['status'], kept['status'] | B.buf['status']), t
        sb = B.get_state()
        assert torch.equal(A.get_state(), sb), t
        term = ia['terminal_observation']
        for k in OBS:
            assert torch.equal(term[k][mask], kept[k][mask]), (t, k)
        assert torch.equal(ia['terminal_status'][mask], kept['status'][mask]), t
        assert torch.equal(A.episode_steps, cnt), t
        used = sb[:, col].contiguous().view(torch.int32) - rng0
        assert not bool(used[~mask].any()), t
        draws.append(used[mask].cpu())
    return ends, torch.cat(draws).tolist()


@pytest.mark.parametrize('gid', IDS)
def test_autoreset_equals_step_then_masked_reset_bitwise(gid):
    """handle A: rp_step_autoreset with a time limit of 4 (counters staggered e % 4), a random 5 % end_mask and the fault rule; twin B: rp_step, rows
    kept, rp_reset(mask of the envs that ended).  A's observations, the pack's observation part and every state row (record + contact cache) equal B's
    after its reset; A's reward / is_success / target_poses and the pack's last two columns equal B's step rows; A's status = B's step status | its
    reset status; terminal_observation = B's step rows; done = the expected mask; the counters follow."""
    n, steps, seed = 256, 20, 11
    A = make(gid, n, seed, autoreset=True, max_episode_steps=4)
    B = make(gid, n, seed)
    A.reset(); B.reset()
    ends, _ = compare_with_twin(A, B, steps, seed, 4)
    ended = sum(ends)
    assert ended > n * steps // 5, ended           # the time limit alone ends a quarter of the envs every step


def autoreset_shape(env):
    grid, epb = C.c_int32(), C.c_int32()
    assert env.lib.rp_debug_autoreset_shape(env.h, C.byref(grid), C.byref(epb)) == 0
    return grid.value, epb.value


SHAPES = ((None, 2), (None, 4), (1, 1), (1, 4), (3, 3), (7, 2))
N_SMALL, N_LARGE = 100, 4196


@pytest.mark.parametrize('blocks,epb', SHAPES, ids=['blocks%s-epb%d' % (b or 'default', e) for b, e in SHAPES])
@pytest.mark.parametrize('gid', tuple(DRAWS))
def test_shared_blocks_refilled_slots_and_retries_bitwise(gid, blocks, epb, monkeypatch):
    """k_autoreset off its one-env-per-block path: RP_AUTORESET_BLOCKS / RP_AUTORESET_EPB set for handle A only, the same comparison with twin B as
    test_autoreset_equals_step_then_masked_reset_bitwise, and two steps in which every env ends.

    There the ends outnumber the grid's slots (grid x epb, read back with rp_debug_autoreset_shape), so slots are refilled from the list after their env
    is done.  With the default grid that takes more envs than the blocks resident at once hold (MI355X: 1024 blocks): N = 4196, otherwise N = 100; both
    leave k_autoreset_mark's last wave partial.  Every ended env's reset is decoded from its RNG draws (tests/reset_draws.py) into extra attempts (a
    solved sparse goal: the whole reset again) and object re-samples (depth: settled out of bounds); both retry branches must have been compared bit
    for bit.  Measured on the MI355X, seed 11 (the same in every shape: the draws do not depend on the launch shape), envs with attempt > 0 / with
    depth > 0 among the ends:
        N = 4196 (8828 ends)   U: 2856 / 0      P: 5 / 190     W: 5086 / 323
        N = 100  (212 ends)    U: 72 / 0        P: 0 / 2       W: 108 / 4
    So the attempt branch is asserted for U and W in every shape and for P at N = 4196 (epb 2, 4); the depth branch for P and W in every shape.  U
    settled no object out of bounds in 9040 device resets (the oracle: none in 300), so U's depth branch is left to
    test_refilled_slot_starts_its_own_resample_count."""
    big = blocks is None
    n = N_LARGE if big else N_SMALL
    steps, seed, stagger, full_ends = (4, 11, 4, (0, 2)) if big else (5, 11, 4, (0, 3))
    monkeypatch.delenv('RP_AUTORESET_BLOCKS', raising=False)
    monkeypatch.delenv('RP_AUTORESET_EPB', raising=False)
    B = make(gid, n, seed)
    if blocks is not None:
        monkeypatch.setenv('RP_AUTORESET_BLOCKS', str(blocks))
    monkeypatch.setenv('RP_AUTORESET_EPB', str(epb))
    A = make(gid, n, seed, autoreset=True, max_episode_steps=stagger)
    grid_b, epb_b = autoreset_shape(B)
    assert epb_b == 1 and 1 <= grid_b <= n, (grid_b, epb_b)
    grid, got_epb = autoreset_shape(A)
    assert got_epb == epb and (blocks is None or grid == blocks), (grid, got_epb)
    A.reset(); B.reset()
    ends, draws = compare_with_twin(A, B, steps, seed, stagger, full_ends)
    per_attempt, per_resample = DRAWS[gid]
    decoded = [decode(d, per_attempt, per_resample) for d in draws]
    assert None not in decoded, sorted(set(d for d, x in zip(draws, decoded) if x is None))
    retried = sum(a > 0 for a, _ in decoded)
    resampled = sum(s > 0 for _, s in decoded)
    beyond = sum(max(0, x - grid * epb) for x in ends)
    print('%s blocks=%s: grid %d, epb %d, N %d, ends %d (per step %s), ends beyond grid x epb %d, envs with attempt > 0: %d, with depth > 0: %d, '
          'draws %s' % (gid, blocks, grid, epb, n, sum(ends), ends, beyond, retried, resampled, sorted(collections.Counter(draws).items())))
    for t in full_ends:
        assert ends[t] == n and ends[t] > grid * epb, (t, ends[t], grid, epb)
    if gid != 'pandaPick-v0' or big:
        assert retried > 0, retried
    if gid != 'UR5PlayAbsRPY1Obj-v0':
        assert resampled > 0, resampled


def test_no_ends_equals_rp_step_bitwise():
    """without a time limit, mask or fault the autoreset step is rp_step: same outputs and state for 20 steps, and the counters read 20"""
    n, steps, seed = 64, 20, 4
    A = make('UR5PlayAbsRPY1Obj-v0', n, seed, autoreset=True, max_episode_steps=0)
    B = make('UR5PlayAbsRPY1Obj-v0', n, seed)
    A.reset(); B.reset()
    acts = actions(A, steps, seed)
    for t in range(steps):
        oa, ra, da, ia = A.step(acts[t])
        ob, rb, _, ib = B.step(acts[t])
        torch.cuda.synchronize()
        assert not bool(da.any()), t
        for k in OBS:
            assert torch.equal(oa[k], ob[k]), (t, k)
        for k in ('is_success', 'target_poses', 'status'):
            assert torch.equal(ia[k], ib[k]), (t, k)
        assert torch.equal(ra, rb) and torch.equal(A.pack, B.pack), t
    assert torch.equal(A.get_state(), B.get_state())
    assert torch.equal(A.episode_steps, torch.full((n,), steps, dtype=torch.int32, device=A.device))


def test_fault_ends_the_episode():
    """a block put below the ground plate (set_state) faults its env (status bit 2): the env ends with reason 4, its terminal status carries bit 2, and
    the new episode's observation is finite"""
    n = 32
    A = make('UR5PlayAbsRPY1Obj-v0', n, 2, autoreset=True, max_episode_steps=0)
    A.reset()
    s = A.get_state()
    z = A.state_layout['free0'][0] + 2
    bad = torch.tensor([3, 10, 20], device=A.device)
    s[bad, z] = -1.0
    A.set_state(s)
    obs, _, done, info = A.step(actions(A, 1, 3)[0])
    torch.cuda.synchronize()
    want = torch.zeros(n, dtype=torch.bool, device=A.device)
    want[bad] = True
    assert torch.equal(done, want)
    assert torch.equal(info['done_reason'][bad], torch.full((3,), 4, dtype=torch.int32, device=A.device))
    assert bool(((info['terminal_status'][bad] & 2) != 0).all())
    assert float(info['terminal_observation']['achieved_goal'][bad, 2].max()) < 0.0
    for k in OBS[:-1]:
        assert bool(torch.isfinite(obs[k]).all()), k
    assert float(obs['achieved_goal'][bad, 2].min()) > -0.2          # back on the table
    assert bool((A.episode_steps[bad] == 0).all()) and bool((A.episode_steps[~want] == 1).all())


def test_success_ends_the_episode():
    """end_on_success: with the goal put on the achieved goal (set_state) in half of the envs, done bit 8 is exactly the transition's is_success"""
    n = 32
    A = make('UR5PlayAbsRPY1Obj-v0', n, 6, autoreset=True, max_episode_steps=0, end_on_success=True)
    obs = A.reset()
    s = A.get_state()
    g0 = A.state_layout['goal'][0]
    na = A.dims['achieved_goal']
    s[:, g0:g0 + na] = obs['achieved_goal']
    s[n // 2:, g0] += 0.3                                               # the other half stays unsolved
    A.set_state(s)
    obs, _, done, info = A.step(actions(A, 1, 9)[0])
    torch.cuda.synchronize()
    succ = info['is_success'] != 0
    assert int(succ.sum()) >= n // 4, int(succ.sum())
    assert not bool(succ[n // 2:].any())
    assert torch.equal((info['done_reason'] & 8) != 0, succ)
    assert torch.equal(done, info['done_reason'] != 0)
    for k in OBS[:-1]:
        assert bool(torch.isfinite(obs[k]).all()), k


def _rollout(env, steps, seed, masks, stagger):
    env.reset()
    env.episode_steps = torch.arange(env.num_envs, dtype=torch.int32) % stagger
    acts = actions(env, steps, seed)
    rows = []
    for t in range(steps):
        obs, r, done, info = env.step(acts[t], end_mask=masks[t])
        rows.append(tuple(obs[k].clone() for k in OBS) + (r.clone(), done.clone(), info['status'].clone(), env.get_state()))
    torch.cuda.synchronize()
    return rows


def test_pipelines_and_groups_give_the_same_bits():
    """split pipeline with one and three groups, k_step (fused 1) and k_chain (fused 2): the same bits with ends in every step"""
    n, steps, seed = 64, 8, 21
    runs = []
    for fused, groups in ((0, 1), (0, 3), (1, 1), (2, 1)):
        env = make('pandaPick-v0', n, seed, autoreset=True, max_episode_steps=3)
        env.set_groups(groups)
        env.set_fused(fused)
        runs.append(_rollout(env, steps, seed, end_masks(n, steps, seed, env.device, 0.1), 3))
        env.close()
    for run in runs[1:]:
        for t in range(steps):
            for x, y in zip(runs[0][t], run[t]):
                assert torch.equal(x, y), t


def test_one_handle_equals_two_shards():
    """one handle of 2n envs == handles of n envs with env_offset 0 and n"""
    n, steps, seed = 32, 8, 5
    full = make('UR5PlayAbsRPY1Obj-v0', 2 * n, seed, autoreset=True, max_episode_steps=3)
    a = make('UR5PlayAbsRPY1Obj-v0', n, seed, env_offset=0, autoreset=True, max_episode_steps=3)
    b = make('UR5PlayAbsRPY1Obj-v0', n, seed, env_offset=n, autoreset=True, max_episode_steps=3)
    for env in (full, a, b):
        env.reset()
    e = torch.arange(2 * n, dtype=torch.int32)
    full.episode_steps = e % 3
    a.episode_steps = e[:n] % 3
    b.episode_steps = e[n:] % 3
    acts = actions(full, steps, seed)
    masks = end_masks(2 * n, steps, seed, full.device, 0.1)
    for t in range(steps):
        of, rf, df, _ = full.step(acts[t], end_mask=masks[t])
        of = {k: v.clone() for k, v in of.items() if v is not None}
        rf, df = rf.clone(), df.clone()
        oa, ra, da, _ = a.step(acts[t, :n], end_mask=masks[t][:n])
        ob, rb, db, _ = b.step(acts[t, n:], end_mask=masks[t][n:])
        torch.cuda.synchronize()
        for k in OBS:
            assert torch.equal(of[k], torch.cat([oa[k], ob[k]])), (t, k)
        assert torch.equal(rf, torch.cat([ra, rb])) and torch.equal(df, torch.cat([da, db])), t
    assert torch.equal(full.get_state(), torch.cat([a.get_state(), b.get_state()]))
    assert torch.equal(full.episode_steps, torch.cat([a.episode_steps, b.episode_steps]))


def test_step_returns_before_the_gpu_is_done():
    """nothing in the autoreset step waits for the device: behind a ~1 s sleep kernel on the stream, step (with every env ending) returns while the
    stream is still busy"""
    n = 64
    env = make('UR5PlayAbsRPY1Obj-v0', n, 8, autoreset=True, max_episode_steps=0)
    env.reset()
    act = actions(env, 1, 8)[0]
    ends = torch.ones(n, dtype=torch.uint8, device=env.device)
    stream = torch.cuda.current_stream(env.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))      # ~1 s of the sleep kernel's clock
    torch.cuda._sleep(cycles)
    _, _, done, _ = env.step(act, end_mask=ends)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    assert bool(done.all())


@pytest.mark.parametrize('blocks,epb', ((3, 3), (7, 2)), ids=('blocks3-epb3', 'blocks7-epb2'))
@pytest.mark.parametrize('gid', tuple(DRAWS))
def test_refilled_slot_starts_its_own_resample_count(gid, blocks, epb, monkeypatch):
    """every object sample settles out of bounds (env_range_high's z below the table), so every attempt of every reset runs into the depth cap: 9
    samples, per_attempt + 8 x per_resample draws.  A slot refilled after such an env must start the next env at depth 0 - one that kept the old slot's
    depth 8 would sample once and differ from twin B (same ranges) and from the draw count.  Seed 11, N = 100, grid x epb = 9 / 14, two steps in which
    all envs end, one with the time limit's quarter.  Measured (draws: count): U 35: 141, 70: 41, 105: 16, 140: 4; P 33: 202; W 65: 82, 130: 50, ...
    up to 780 (12 attempts)."""
    n, steps, seed, stagger = 100, 3, 11, 4
    hi = [1.0, 1.0, -1.0]
    monkeypatch.delenv('RP_AUTORESET_BLOCKS', raising=False)
    monkeypatch.delenv('RP_AUTORESET_EPB', raising=False)
    B = make(gid, n, seed, env_range_high=hi)
    monkeypatch.setenv('RP_AUTORESET_BLOCKS', str(blocks))
    monkeypatch.setenv('RP_AUTORESET_EPB', str(epb))
    A = make(gid, n, seed, env_range_high=hi, autoreset=True, max_episode_steps=stagger)
    grid, got_epb = autoreset_shape(A)
    assert (grid, got_epb) == (blocks, epb)
    A.reset(); B.reset()
    ends, draws = compare_with_twin(A, B, steps, seed, stagger, (0, 2))
    per_attempt, per_resample = DRAWS[gid]
    capped = per_attempt + 8 * per_resample
    print('%s blocks=%d epb=%d: ends %s, draws %s' % (gid, blocks, epb, ends, sorted(collections.Counter(draws).items())))
    assert ends[0] == ends[2] == n and n > grid * epb
    assert all(d > 0 and d % capped == 0 for d in draws), sorted(set(draws))
