"""The draw arithmetic tests/test_gpu_autoreset.py decodes k_autoreset's retries with (tests/reset_draws.py), held against the CPU oracle.

Seed 11, the first two resets of envs 0 .. 149 (OracleEnv(..., f32=True).reset(), last_used), draws: count
    UR5PlayAbsRPY1Obj-v0   11: 214, 22: 58, 33: 19, 44: 8, 55: 1
    pandaPick-v0           9: 299, 12: 1                      (envs 0 .. 1999: 9: 3977, 12: 22, 18: 1)
    pandaPlay-v0           17: 130, 34: 73, 51: 45, 68: 22, 85: 10, 102: 9, 119: 1, 136: 5, 153: 3, 170: 1, 238: 1
"""
import pytest

from oracle import OracleEnv
from reset_draws import DRAWS, decode, draws_per_reset

SEED, ENVS = 11, 150


@pytest.mark.parametrize('gid', sorted(DRAWS))
def test_per_attempt_and_per_resample_draws_match_the_oracle(gid):
    """the constants come from the scene (objects, play), and the oracle spends exactly them: a dense-reward reset is one attempt (11 / 9 / 17 draws);
    with the env's upper bound below the table every sample settles out of bounds, so a one-object reset samples 9 times (depth 8): per_attempt + 8 x
    per_resample.  (The oracle's two-object reset recurses per object - out of scope here - but every one of its samples still costs per_resample.)"""
    per_attempt, per_resample = DRAWS[gid]
    o = OracleEnv(gid, seed=SEED, f32=True)
    f = o.flags()
    assert (per_attempt, per_resample) == draws_per_reset(f['num_objects'], bool(f['play']))
    dense = OracleEnv(gid, seed=SEED, f32=True, dense_reward=True)
    dense.reset()
    assert dense.last_used == per_attempt
    r = o.ranges()
    low = OracleEnv(gid, seed=SEED, f32=True, dense_reward=True, ranges=[r[k] for k in ('goal_lo', 'goal_hi', 'obj_lo', 'obj_hi')] + [[-9.0] * 3])
    low.reset()
    if f['num_objects'] == 1:
        assert low.last_used == per_attempt + 8 * per_resample
    else:
        assert low.last_used > per_attempt + 8 * per_resample and (low.last_used - per_attempt) % per_resample == 0


@pytest.mark.parametrize('gid', sorted(DRAWS))
def test_oracle_reset_draws_decode_into_whole_attempts_and_resamples(gid):
    """every reset's draw count is whole attempts and re-samples; the pinned seed has resets that took more than one attempt (U, W: 86 and 170 of
    300) and one that re-sampled the object (P: env 24, its second reset, 12 draws = one attempt + one re-sample)"""
    per_attempt, per_resample = DRAWS[gid]
    retried, resampled = [], []
    for e in range(ENVS):
        o = OracleEnv(gid, seed=SEED, env_index=e, f32=True)
        for k in range(2):
            o.reset()
            d = decode(o.last_used, per_attempt, per_resample)
            assert d is not None, (e, k, o.last_used)
            attempt, resamples = d
            assert (attempt + 1) * per_attempt + resamples * per_resample == o.last_used
            assert resamples <= 8 * (attempt + 1), (e, k, o.last_used)
            if attempt > 0:
                retried.append((e, k))
            if resamples > 0:
                resampled.append((e, k))
    if gid == 'pandaPick-v0':
        assert (24, 1) in resampled, resampled
        assert decode(12, per_attempt, per_resample) == (0, 1)
    else:
        assert len(retried) >= 50, len(retried)
        assert decode(2 * per_attempt, per_attempt, per_resample) == (1, 0)
    assert decode(per_attempt - 1, per_attempt, per_resample) is None
