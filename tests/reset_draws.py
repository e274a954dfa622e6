"""How many RNG draws one reset takes, and the decoding of a reset's draw count into attempts and object re-samples.

A reset (rp_reset, k_autoreset, the oracle's rpo_reset) draws from the counter RNG whose counter is the record's ST_RNG (csrc/rp_device_model.h):
  - reset_sample_objects: 3 per object (its spawn position);
  - reset_sample_arm_target: 3 (the arm's IK target);
  - reset_goal_pos: 3 per goal (max(num_objects, 1) goals), and in a play scene 2 more (which goal coordinate to bump, and the bump).
One attempt is one object sample, the arm target and the goal.  An object that settles out of bounds is sampled again (depth + 1, at most 8 per attempt);
a sparse goal that is already solved starts the whole attempt again (attempt + 1).  So a reset with `a` extra attempts and `s` re-samples in all draws
    (a + 1) * per_attempt + s * per_resample.
"""
from math import gcd

RNG_COL = {False: 116, True: 125}           # ST_RNG in the record (the RP_WIDE build: 125), an int32 bit pattern


def draws_per_reset(num_objects, play):
    """(draws of one attempt, draws of one object re-sample)"""
    per_resample = 3 * num_objects
    return per_resample + 3 + 3 * max(num_objects, 1) + (2 if play else 0), per_resample


# U: UR5 one-object play scene; P: pandaPick (no play scene); W: the two-object play scene (wide build)
DRAWS = {'UR5PlayAbsRPY1Obj-v0': draws_per_reset(1, True), 'pandaPick-v0': draws_per_reset(1, False), 'pandaPlay-v0': draws_per_reset(2, True)}


def decode(draws, per_attempt, per_resample):
    """(extra attempts, object re-samples) of a reset that took `draws` draws, or None if no whole number of attempts and re-samples makes it.

    Of the decompositions the one with the fewest re-samples is taken (0 <= s < per_attempt / g, g = gcd): that is the true one while a reset re-samples
    fewer than per_attempt / g times in all (U: 11, W: 17, P: 3).  Beyond that, a decoded s > 0 still proves a re-sample (the true s equals it modulo
    per_attempt / g)."""
    for s in range(per_attempt // gcd(per_attempt, per_resample)):
        rest = draws - s * per_resample
        if rest >= per_attempt and rest % per_attempt == 0:
            return rest // per_attempt - 1, s
    return None
