"""rp_set_reset_table: rp_step_autoreset restarts the ended envs from rows of a device table with rp_reset_to's semantics.  Run with -m gpu on the
MI355X box.

The yardstick is a twin handle with the same seed that runs rp_step, keeps the rows, and then rp_reset_to with the table rows that the rule of
tests/reset_rows.py gives the envs that should have ended.  reset(o) draws only from the env's own counter RNG, so the two must agree bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from reset_rows import reset_rows
from test_gpu_autoreset import OBS, actions, compare_with_twin, end_masks, make

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

IDS = ('UR5PlayAbsRPY1Obj-v0', 'pandaPick-v0', 'UR5Reach-v0', 'pandaPlay-v0')
N = 1101                                   # 18 waves, the last one partial
WAVE_EDGES = (0, 63, 64, 1000, N - 1)
READS = {'pandaPlay-v0': 28}               # entries of o that reset(o) reads where obs_quat is shorter (two blocks: o[21:28]; obs_quat has 26)


def start_table(env, rows, seed):
    """random_start_table's rows, zero-padded to what reset(o) reads"""
    t = env.random_start_table(rows, seed)
    assert t.shape == (rows, env.dims['obs_quat'])
    pad = READS.get(env.env_id, 0) - t.shape[1]
    return torch.cat([t, torch.zeros((rows, pad), dtype=t.dtype, device=t.device)], 1) if pad > 0 else t


def compare_with_reset_to_twin(A, B, table, steps, seed, stagger, cursor=0, edge_steps=()):
    """A: rp_step_autoreset with `table` set (time limit = stagger, counters staggered e % stagger, a random 5 % end_mask - plus envs WAVE_EDGES in
    the steps `edge_steps` - and the fault rule); twin B: rp_step, rows kept, rp_reset_to(table[r(e)], mask of the envs that ended), r from the row
    rule.  Every state row (record + contact cache), the observations, the pack, reward / is_success / target_poses / status under the autoreset rules,
    terminal_observation, done, done_reason, the counters and info['reset_row'] must agree.  Returns the ends of every step and the cursor."""
    n = A.num_envs
    dev = A.device
    e = torch.arange(n, device=dev, dtype=torch.int32)
    A.episode_steps = e % stagger
    cnt = (e % stagger).clone()
    acts = actions(A, steps, seed)
    masks = end_masks(n, steps, seed + 1, dev)
    for t in edge_steps:
        masks[t][list(WAVE_EDGES)] = 1
    no, na = A.dims['obs_quat'], A.dims['achieved_goal']
    rows = table.shape[0]
    ends = []
    for t in range(steps):
        oa, ra, da, ia = A.step(acts[t], end_mask=masks[t])
        B.step(acts[t])
        kept = {k: B.buf[k].clone() for k in OBS + ('reward', 'is_success', 'target_poses', 'status')}
        kept_pack = B.pack.clone()
        c1 = cnt + 1
        reason = (c1 >= stagger).int() | (masks[t] != 0).int() * 2 | ((kept['status'] & 3) != 0).int() * 4
        mask = reason != 0
        cnt = torch.where(mask, torch.zeros_like(c1), c1)
        r, cursor = reset_rows(mask.cpu().numpy(), cursor, rows)
        r = torch.from_numpy(r).to(dev)
        if bool(mask.any()):
            B.reset(mask=mask, o=table[r.clamp(min=0).long()])
        torch.cuda.synchronize()
        ends.append(int(mask.sum()))
        assert torch.equal(da, mask), t
        assert torch.equal(ia['done_reason'], reason), t
        assert torch.equal(ia['reset_row'], r), t
        for k in OBS:
            assert torch.equal(oa[k], B.buf[k]), (t, k)
        assert torch.equal(A.pack[:, :no + na], B.pack[:, :no + na]), t
        assert torch.equal(A.pack[:, no + na:], kept_pack[:, no + na:]), t
        assert torch.equal(ra, kept['reward']), t
        assert torch.equal(ia['is_success'], kept['is_success']), t
        assert torch.equal(ia['target_poses'], kept['target_poses']), t
        assert torch.equal(ia['status'], kept['status'] | B.buf['status']), t
        assert torch.equal(A.get_state(), B.get_state()), t
        term = ia['terminal_observation']
        for k in OBS:
            assert torch.equal(term[k][mask], kept[k][mask]), (t, k)
        assert torch.equal(ia['terminal_status'][mask], kept['status'][mask]), t
        assert torch.equal(A.episode_steps, cnt), t
    return ends, cursor


@pytest.mark.parametrize('size', ('wrap', 'beyond_n'))
@pytest.mark.parametrize('gid', IDS)
def test_table_autoreset_equals_step_then_reset_to_bitwise(gid, size):
    """30 steps, a time limit of 8 (about N / 8 ends per step), a random end_mask, ends in five waves at steps 3 and 17; a table of 7 rows (every
    step's ends wrap it) or of N + 37 rows (rows > N: the cursor runs on past N and wraps between steps)."""
    steps, seed, stagger = 30, 13, 8
    B = make(gid, N, seed)
    rows = 7 if size == 'wrap' else N + 37
    table = start_table(B, rows, seed + 100)
    A = make(gid, N, seed, autoreset=True, max_episode_steps=stagger, reset_table=table)
    A.reset(); B.reset()
    ends, cursor = compare_with_reset_to_twin(A, B, table, steps, seed, stagger, edge_steps=(3, 17))
    assert min(ends) > 0
    if size == 'wrap':
        assert min(ends) > rows, ends
    else:
        assert sum(ends) > rows, (sum(ends), rows)          # the cursor wrapped
    print('%s %s: ends %s, cursor %d' % (gid, size, ends, cursor))


def _rollout(env, table, steps, seed, masks, stagger):
    env.reset()
    env.set_reset_table(table)
    env.episode_steps = torch.arange(env.num_envs, dtype=torch.int32) % stagger
    acts = actions(env, steps, seed)
    rows = []
    for t in range(steps):
        obs, r, done, info = env.step(acts[t], end_mask=masks[t])
        rows.append(tuple(obs[k].clone() for k in OBS) + (r.clone(), done.clone(), info['status'].clone(), info['reset_row'].clone(), env.pack.clone(),
                                                         env.get_state()))
    torch.cuda.synchronize()
    return rows


@pytest.mark.parametrize('gid', ('pandaPick-v0', 'UR5PlayAbsRPY1Obj-v0'))
def test_pipelines_groups_and_repeats_give_the_same_bits(gid):
    """split pipeline with the default groups and with one, k_step (fused 1) and k_chain (fused 2), and the default once more: the same bits with a
    table and ends in every step"""
    n, steps, seed = 200, 8, 21
    table = make(gid, 8, seed).random_start_table(37, seed)
    runs = []
    for fused, groups in ((0, None), (0, 1), (1, None), (2, None), (0, None)):
        env = make(gid, n, seed, autoreset=True, max_episode_steps=3)
        if groups is not None:
            env.set_groups(groups)
        env.set_fused(fused)
        runs.append(_rollout(env, table, steps, seed, end_masks(n, steps, seed, env.device, 0.1), 3))
        env.close()
    assert all(bool(run[t][-5].any()) for run in runs for t in range(steps))
    for run in runs[1:]:
        for t in range(steps):
            for x, y in zip(runs[0][t], run[t]):
                assert torch.equal(x, y), t


def test_removing_the_table_returns_to_the_settle_path():
    """steps with a table, then set_reset_table(None): twin B takes A's state, and autoreset equals step + rp_reset(mask) bit for bit again
    (test_gpu_autoreset's compare_with_twin); reset_row is -1 everywhere"""
    gid, n, seed = 'UR5PlayAbsRPY1Obj-v0', 256, 17
    A = make(gid, n, seed, autoreset=True, max_episode_steps=4)
    A.set_reset_table(A.random_start_table(11, seed))
    A.reset()
    A.episode_steps = torch.arange(n, dtype=torch.int32) % 4
    acts = actions(A, 4, seed + 5)
    for t in range(4):
        _, _, done, info = A.step(acts[t])
        assert bool(done.any()) and bool((info['reset_row'][done] >= 0).all()), t
    A.set_reset_table(None)
    B = make(gid, n, seed)
    B.reset()
    B.set_state(A.get_state())
    torch.cuda.synchronize()
    ends, _ = compare_with_twin(A, B, 6, seed, 4)
    assert sum(ends) > n, ends
    _, _, done, info = A.step(acts[0])
    assert bool(done.any()) and bool((info['reset_row'] == -1).all())


def _ranks_from(env, cursor, rows, act, ends_at):
    mask = torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device)
    mask[list(ends_at)] = 1
    _, _, done, info = env.step(act, end_mask=mask)
    torch.cuda.synchronize()
    want, cursor = reset_rows(done.cpu().numpy(), cursor, rows)
    assert torch.equal(info['reset_row'].cpu(), torch.from_numpy(want))
    return cursor


def test_cursor_lifecycle():
    """a new table starts at row 0; rp_reset and rp_reset_to leave the cursor where it was"""
    gid, n, seed = 'pandaPick-v0', 130, 3
    A = make(gid, n, seed, autoreset=True, max_episode_steps=0, end_on_fault=False)
    table = A.random_start_table(5, seed)
    A.reset()
    A.set_reset_table(table)
    act = actions(A, 1, seed)[0]
    cur = _ranks_from(A, 0, 5, act, (1, 70, 129))
    assert cur == 3
    cur = _ranks_from(A, cur, 5, act, (2, 3))
    assert cur == 0
    cur = _ranks_from(A, cur, 5, act, (4, 64, 65))
    assert cur == 3
    A.set_reset_table(table[:4].clone())                # a new table: the cursor is 0 again
    cur = _ranks_from(A, 0, 4, act, (0, 127))
    assert cur == 2
    some = torch.zeros(n, dtype=torch.uint8, device=A.device)
    some[5:40] = 1
    A.reset(mask=some)
    A.reset(mask=some, o=A.buf['obs_quat'].clone())
    cur = _ranks_from(A, cur, 4, act, (10, 20, 30))     # rows 2, 3, 0: the resets did not move the cursor
    assert cur == 1


def test_table_without_ends_equals_rp_step_bitwise():
    """with a table set and no ends, the autoreset step is rp_step: same outputs and state for 12 steps; reset_row stays -1"""
    n, steps, seed = 64, 12, 4
    A = make('UR5PlayAbsRPY1Obj-v0', n, seed, autoreset=True, max_episode_steps=0)
    A.set_reset_table(A.random_start_table(9, seed))
    B = make('UR5PlayAbsRPY1Obj-v0', n, seed)
    A.reset(); B.reset()
    acts = actions(A, steps, seed)
    for t in range(steps):
        oa, ra, da, ia = A.step(acts[t])
        ob, rb, _, ib = B.step(acts[t])
        torch.cuda.synchronize()
        assert not bool(da.any()) and bool((ia['reset_row'] == -1).all()), t
        for k in OBS:
            assert torch.equal(oa[k], ob[k]), (t, k)
        for k in ('is_success', 'target_poses', 'status'):
            assert torch.equal(ia[k], ib[k]), (t, k)
        assert torch.equal(ra, rb) and torch.equal(A.pack, B.pack), t
    assert torch.equal(A.get_state(), B.get_state())


@pytest.mark.parametrize('gid,need', (('UR5PlayAbsRPY1Obj-v0', 18), ('pandaPlay-v0', 28), ('UR5Reach-v0', 3)))
def test_bad_tables_are_refused(gid, need):
    """n_o below what rp_reset_to reads, on both builds, and rows < 0: -1 with a message that names the numbers; the handle keeps working"""
    env = make(gid, 8, 1, autoreset=True, max_episode_steps=0)
    lib, stream = env.lib, env._stream()
    t = torch.zeros((4, need), dtype=torch.float32, device=env.device)
    assert lib.rp_set_reset_table(env.h, C.c_void_p(t.data_ptr()), 4, need - 1, stream) == -1
    msg = lib.rp_last_error(env.h).decode()
    assert str(need - 1) in msg and str(need) in msg, msg
    assert lib.rp_set_reset_table(env.h, C.c_void_p(t.data_ptr()), -2, need, stream) == -1
    assert '-2' in lib.rp_last_error(env.h).decode()
    with pytest.raises(RuntimeError):
        env.set_reset_table(t[:, :need - 1])
    assert lib.rp_set_reset_table(env.h, C.c_void_p(t.data_ptr()), 4, need, stream) == 0
    assert lib.rp_set_reset_table(env.h, None, 0, 0, stream) == 0


def test_step_with_a_table_returns_before_the_gpu_is_done():
    """behind a ~1 s sleep kernel on the stream, an autoreset step with a table and every env ending returns while the stream is still busy"""
    n = 64
    env = make('UR5PlayAbsRPY1Obj-v0', n, 8, autoreset=True, max_episode_steps=0)
    env.set_reset_table(env.random_start_table(16, 8))
    env.reset()
    act = actions(env, 1, 8)[0]
    ends = torch.ones(n, dtype=torch.uint8, device=env.device)
    stream = torch.cuda.current_stream(env.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); torch.cuda._sleep(10 ** 7); t1.record()
    torch.cuda.synchronize()
    cycles = int(min(10 ** 7 * 1000.0 / max(t0.elapsed_time(t1), 1e-3), 5e9))      # ~1 s of the sleep kernel's clock
    torch.cuda._sleep(cycles)
    _, _, done, info = env.step(act, end_mask=ends)
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy
    assert bool(done.all())
    assert torch.equal(info['reset_row'].cpu(), torch.arange(n, dtype=torch.int32) % 16)


@pytest.mark.parametrize('gid', IDS)
def test_random_start_table_is_the_obs_of_fresh_resets(gid):
    m, seed = 40, 9
    env = make(gid, 4, 0, autoreset=True)
    got = env.random_start_table(m, seed)
    want = make(gid, m, seed).reset()['obs_quat'].clone()
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert np.isfinite(got.cpu().numpy()).all()
