"""The narrowphase's shared caps, CPU only.

The device (csrc/rp_kernels.cuh) and the CPU oracle (oracle/rp_oracle.c) cut the substep's contact work at the same caps in the same order; only comments
tied the two columns together.  Here the preprocessor reads both sides - with the -D flags their Makefiles compile them with - and every cap is pinned
against its counterpart, so a one-sided override (-DS4_SLOTS1=16 on the device, -DMAX_CONTACTS=40 on the oracle) fails.  The scene generator of the GPU
cap tests (tests/crowded_scenes.py) is held to the caps it is meant to reach, per id, through the oracle's own counters (rpo_last_collide_counts)."""
import ctypes as C
import os
import re
import shlex
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'roboticsplayroompybullet_amd', 'csrc')
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, 'oracle'), os.path.dirname(os.path.abspath(__file__))) if p not in sys.path]
import cache_rows  # noqa: E402
import crowded_scenes  # noqa: E402

# (device macro, oracle macro, what is cut)
PINS = [('MAXACT', 'MAX_ACTIVE_PAIRS', 'AABB-overlapping pairs examined, in pair order'),
        ('CANDMAX', 'MAX_CANDIDATES', 'candidate points, pairs in order'),
        ('PM_MAX', 'PM_MAX', 'cached manifolds'),
        ('MAXC', 'MAX_CONTACTS', 'contacts passed to the solver'),
        ('MAXT', 'MAX_TORS', 'torsional friction rows'),
        ('S4_SLOTS0', 'RES_SLOTS0', 'four-env path slots of the row-0 stream / residual form'),
        ('S4_SLOTS1', 'RES_SLOTS1', 'four-env path slots of the row-1 stream / residual form'),
        ('PMC_AXN', 'GJK_AX', 'cached GJK results per env'),
        ('PMC_FLOATS', 'RPO_ROW_WORDS', 'words of a contact-cache row')]
# which counter of rpo_last_collide_counts each cap bounds
COUNTED = {'pairs': ('MAXACT', 'MAX_ACTIVE_PAIRS'), 'candidates': ('CANDMAX', 'MAX_CANDIDATES'), 'manifolds': ('PM_MAX', 'PM_MAX'),
           'contacts': ('MAXC', 'MAX_CONTACTS'), 'torsional': ('MAXT', 'MAX_TORS')}


def _gcc():
    for cc in ('gcc', 'cc'):
        try:
            subprocess.run([cc, '--version'], check=True, capture_output=True)
            return cc
        except (OSError, subprocess.CalledProcessError):
            pass
    pytest.skip('no C compiler')


def make_flags(makefile, var):
    """the -D / -U flags of `var ?= ...` in a Makefile (what the build compiles that side with)"""
    txt = open(makefile).read()
    m = re.search(r'^%s\s*\??=\s*(.*)$' % var, txt, re.M)
    assert m, (makefile, var)
    return [f for f in shlex.split(m.group(1)) if f.startswith(('-D', '-U'))]


def macros(path, lang, flags, stub):
    """{name: integer value} of every object-like macro defined after preprocessing `path` with `flags` (gcc -E -dM) that evaluates to an integer"""
    out = subprocess.run([_gcc(), '-E', '-dM', '-x', lang, '-I', stub] + list(flags) + [path], check=True, capture_output=True, text=True).stdout
    raw = {}
    for line in out.splitlines():
        m = re.match(r'#define ([A-Za-z_]\w*) (.*)$', line)
        if m:
            raw[m.group(1)] = m.group(2).strip()
    vals = {}

    def ev(name, depth=0):
        if name in vals:
            return vals[name]
        if depth > 20 or name not in raw:
            return None
        expr = raw[name]
        for ident in set(re.findall(r'[A-Za-z_]\w*', expr)):
            v = ev(ident, depth + 1)
            if v is None:
                return None
            expr = re.sub(r'\b%s\b' % ident, '(%d)' % v, expr)
        if not re.fullmatch(r'[\d\s()+\-*/<>|&]+', expr):
            return None
        try:
            vals[name] = int(eval(expr.replace('/', '//')))      # integer arithmetic only (checked above)
        except Exception:
            return None
        return vals[name]
    for k in raw:
        ev(k)
    return vals


@pytest.fixture(scope='module')
def stub(tmp_path_factory):
    """an empty <hip/hip_runtime.h>: the macros of the kernel sources need no HIP toolchain"""
    d = tmp_path_factory.mktemp('stub')
    os.makedirs(d / 'hip')
    (d / 'hip' / 'hip_runtime.h').write_text('')
    return str(d)


def sides(stub, device_extra=(), oracle_extra=(), wide=False, f32=False):
    dev = macros(os.path.join(CSRC, 'rp_kernels.cuh'), 'c++', make_flags(os.path.join(CSRC, 'Makefile'), 'CXXFLAGS') + (['-DRP_WIDE'] if wide else []) + list(device_extra), stub)
    ora = macros(os.path.join(REPO, 'oracle', 'rp_oracle.c'), 'c', make_flags(os.path.join(REPO, 'oracle', 'Makefile'), 'CFLAGS') + (['-DRP_FLOAT'] if f32 else []) + list(oracle_extra), stub)
    return dev, ora


def mismatches(dev, ora):
    bad = [(d, dev.get(d), o, ora.get(o)) for d, o, _ in PINS if dev.get(d) is None or dev.get(d) != ora.get(o)]
    if dev.get('MANPTS') != dev.get('MAXC', -99) + 3:      # the manifold that crosses MAXC is merged whole: MAXC + 3 staged points
        bad.append(('MANPTS', dev.get('MANPTS'), 'MAXC + 3', dev.get('MAXC', -99) + 3))
    return bad


@pytest.mark.parametrize('wide,f32', [(False, False), (True, True), (False, True), (True, False)])
def test_caps_pinned_between_device_and_oracle(stub, wide, f32):
    dev, ora = sides(stub, wide=wide, f32=f32)
    for d, o, what in PINS:
        print('%-11s %4s   %-16s %4s   %s' % (d, dev.get(d), o, ora.get(o), what))
    assert mismatches(dev, ora) == []


def test_cache_row_layout_pinned(stub):
    """PMC_FLOATS == cache_rows.WORDS == rpo_cache_row_words(), PMC_AXN == GJK_AX == cache_rows.AXN, PM_MAX == cache_rows.PM_MAX"""
    import oracle
    dev, ora = sides(stub)
    for f32 in (False, True):
        lib = oracle.load(f32=f32)
        lib.rpo_cache_row_words.restype = C.c_int
        assert dev['PMC_FLOATS'] == cache_rows.WORDS == lib.rpo_cache_row_words() == ora['RPO_ROW_WORDS']
    assert dev['PMC_AXN'] == ora['GJK_AX'] == cache_rows.AXN
    assert dev['PM_MAX'] == ora['PM_MAX'] == cache_rows.PM_MAX
    assert dev['PMC_HDR'] == ora['RPO_ROW_HDR'] == cache_rows.HDR and dev['PMC_PT'] == ora['RPO_ROW_PT'] == cache_rows.PT


def test_generator_caps_are_the_sources(stub):
    dev, ora = sides(stub)
    for name, (d, o) in COUNTED.items():
        assert crowded_scenes.CAPS[name] == dev[d] == ora[o], name


@pytest.mark.parametrize('device_extra,oracle_extra,cap', [(['-DS4_SLOTS1=16'], [], 'S4_SLOTS1'), ([], ['-DMAX_CONTACTS=40'], 'MAXC'),
                                                           ([], ['-DPM_MAX=12'], 'PM_MAX'), (['-DS4_SLOTS0=4'], [], 'S4_SLOTS0')])
def test_one_sided_override_is_caught(stub, device_extra, oracle_extra, cap):
    """the pin reads what the preprocessor makes of each side: an override on one side only is a mismatch"""
    dev, ora = sides(stub, device_extra, oracle_extra)
    bad = mismatches(dev, ora)
    assert any(b[0] == cap for b in bad), bad


def test_makefile_flags_are_read(tmp_path):
    mk = tmp_path / 'Makefile'
    mk.write_text('CXXFLAGS ?= -O3 -std=c++17 -DS4_SLOTS1=16 -ffp-contract=off\n')
    assert make_flags(str(mk), 'CXXFLAGS') == ['-DS4_SLOTS1=16']


def test_oracle_counters_see_the_cut():
    """rpo_last_collide_counts reports what the collision phase wanted: never less than what it kept, and the kept contacts are the cut of the wanted"""
    from oracle import OracleEnv
    for kind in ('U', 'W'):
        for sc in crowded_scenes.generate(kind, 60, seed=3):
            c = sc['counts']
            assert len(sc['contacts']) == min(c['contacts'], crowded_scenes.CAPS['contacts']), (kind, c, len(sc['contacts']))
            assert c['pairs'] >= 0 and c['candidates'] >= 0 and c['manifolds'] >= 0 and c['torsional'] >= 0
    o = OracleEnv('U', seed=7, f32=True)
    o.reset()
    o.contacts()
    first = o.collide_counts()
    o.set_state(o.get_state())
    o.contacts()
    assert o.collide_counts() == first


# Cap coverage of the crowded scenes, per id: the floor of (shallow) scenes that cross each cap the oracle crosses there, and the caps it never crosses
# there (a change that makes one reachable must revisit the GPU cap tests).  Measured with SCENES scenes of seed 0.
SCENES = 1500
FLOORS = {'U': {'manifolds': 8}, 'V': {'manifolds': 1}, 'P': {}, 'W': {'manifolds': 5}}      # (measured: U 11, V 1, W 8)


@pytest.mark.parametrize('kind', ['U', 'V', 'P', 'W'])
def test_crowded_scene_cap_coverage(kind):
    scenes = crowded_scenes.generate(kind, SCENES, seed=0)
    cov = crowded_scenes.coverage(scenes)
    ndeep = sum(sc['deep'] for sc in scenes)
    peak = {k: max(sc['counts'][k] for sc in scenes if not sc['deep']) for k in crowded_scenes.CAPS}
    print('%s (%s): %d scenes, %d deep; scenes that cross each cap %s; peak wanted %s (caps %s)' % (kind, crowded_scenes.IDS[kind], SCENES, ndeep, cov, peak, crowded_scenes.CAPS))
    assert ndeep <= SCENES // 20
    for cap in crowded_scenes.CAPS:
        if cap in FLOORS[kind]:
            assert cov[cap] >= FLOORS[kind][cap], (kind, cap, cov[cap])
        else:
            assert cov[cap] == 0, ('%s: the crowded scenes now cross %s: give it a floor here and check the GPU cap tests cover it' % (kind, cap), cov[cap])
