"""bench.py --dump-outputs, the host half: what a step returned becomes DIR/<name>.npy in float32 / float64, at most 64 MB in all, a larger output cut to
the same seeded rows every time.  No GPU (CPU tensors stand in for the env's buffers); tests/test_gpu_bench_multirank.py runs the flag for real."""
import os

import numpy as np
import torch

import bench


def fake_step(n):
    obs = {'obs_quat': torch.arange(n * 3, dtype=torch.float32).reshape(n, 3), 'img': None,
           'gripper_proprioception': torch.arange(n, dtype=torch.int32)}
    info = {'status': torch.full((n,), 6, dtype=torch.int32), 'target_poses': torch.ones((n, 2), dtype=torch.float32)}
    return obs, torch.linspace(-1, 0, n), torch.zeros(n, dtype=torch.bool), info


def test_host_outputs_names_and_dtypes():
    out = bench.host_outputs(fake_step(5), {'cem_best_return': torch.tensor([1.5, 2.5])})
    assert sorted(out) == ['cem_best_return', 'done', 'info_status', 'info_target_poses', 'obs_gripper_proprioception', 'obs_obs_quat', 'reward']
    assert out['obs_obs_quat'].dtype == np.float32 and out['reward'].dtype == np.float32 and out['info_target_poses'].dtype == np.float32
    assert out['info_status'].dtype == np.float64 and out['done'].dtype == np.float64 and out['obs_gripper_proprioception'].dtype == np.float64
    np.testing.assert_array_equal(out['obs_gripper_proprioception'], np.arange(5))
    np.testing.assert_array_equal(out['info_status'], 6.0)


def test_write_outputs_below_the_cap_writes_every_array_whole(tmp_path):
    arrays = bench.host_outputs(fake_step(64))
    bench.write_outputs(str(tmp_path), dict(arrays))
    assert sorted(os.listdir(tmp_path)) == sorted(k + '.npy' for k in arrays)
    for k, a in arrays.items():
        b = np.load(tmp_path / (k + '.npy'))
        assert b.dtype == a.dtype
        np.testing.assert_array_equal(a, b)


def test_write_outputs_above_the_cap_keeps_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES_MAX', 64 << 10)
    n = 4096
    arrays = bench.host_outputs(fake_step(n), {'gathered_pack': torch.rand((2 * n, 5))})
    assert sum(a.nbytes for a in arrays.values()) > bench.DUMP_BYTES_MAX
    for d in ('a', 'b'):
        bench.write_outputs(str(tmp_path / d), dict(arrays))
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b')) and {'sampled_rows_of_%d.npy' % n, 'sampled_rows_of_%d.npy' % (2 * n)} <= set(files)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= bench.DUMP_BYTES_MAX
    for f in files:
        np.testing.assert_array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))
    for name, rows in (('obs_obs_quat', n), ('gathered_pack', 2 * n)):
        idx = np.load(tmp_path / 'a' / ('sampled_rows_of_%d.npy' % rows)).astype(np.int64)
        assert 0 < len(idx) < rows and (np.diff(idx) > 0).all()
        np.testing.assert_array_equal(np.load(tmp_path / 'a' / (name + '.npy')), arrays[name][idx])
