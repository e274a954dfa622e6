"""Writes tests/golden/arm_truth.json: the slow values of the float64 reference of the dynamics stage (tests/arm_truth.py) on the seeded cases of
tests/arm_cases.py - the bias torque c per case, the end state of each free-fall case, the blocks' end states of each tumbling case - and prints the gaps of both CPU
oracles against them; the fp32 oracle's are what tests/arm_cases.py keeps as FP32_WORST (copy the printed dict there).  CPU only.

    python tools/arm_truth_goldens.py [--check]      (--check: print the gaps from the file as it stands, write nothing)"""
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'oracle'), os.path.join(REPO, 'tests')]
import arm_cases as ac  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from roboticsplayroompybullet_amd import vec_env  # noqa: E402

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'arm_truth.json')


def round_up(x):
    """x at two significant digits, never below it (the CPU test allows no gap above the recorded one)"""
    if x <= 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return float('%.2g' % (math.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e))


def main():
    check = '--check' in sys.argv[1:]
    if check:
        with open(GOLDEN) as f:
            golden = json.load(f)
    else:
        golden = {}
    worst32 = {}
    for kind in ac.IDS:
        model = vec_env._model(kind)
        s0 = ac.scene0(kind)
        if not check:
            golden[kind] = ac.compute_golden(kind, model, s0)
        g = golden[kind]
        cs = ac.cases(kind, model)
        o64, o32 = OracleEnv(ac.IDS[kind], seed=7), OracleEnv(ac.IDS[kind], seed=7, f32=True)
        o64.reset(), o32.reset()
        use = [i for i in range(ac.N_FREEFALL) if ac.usable(cs[i], g['ff'][str(i)]['room'], o64, s0)]
        moving = sum(g['cv_norm'][str(i)] > g['cg_norm'][str(i)] for i in range(ac.N_CASES))
        print('%s: %d of %d free-fall cases usable (not: %s); velocity part of c above its gravity part in %d of %d cases; step check %.1e'
              % (kind, len(use), ac.N_FREEFALL, [i for i in range(ac.N_FREEFALL) if i not in use], moving, ac.N_CASES, max(g['step_check'].values())))
        for name, o in (('fp64', o64), ('fp32', o32)):
            w = ac.oracle_gaps(kind, model, o, g, s0, use)
            print('  %s oracle: %s' % (name, '  '.join('%s %.1e' % (k, w[k]) for k in ac.QUANTITIES + ('acc',))))
            if name == 'fp32':
                worst32[kind] = {k: round_up(w[k]) for k in ac.QUANTITIES}
    print('FP32_WORST = {')
    for kind, w in worst32.items():
        print('    %r: %r,' % (kind, w))
    print('}')
    if not check:
        with open(GOLDEN, 'w') as f:
            json.dump(golden, f, separators=(',', ':'))
            f.write('\n')
        print('wrote %s (%d bytes)' % (os.path.relpath(GOLDEN, REPO), os.path.getsize(GOLDEN)))


if __name__ == '__main__':
    main()
