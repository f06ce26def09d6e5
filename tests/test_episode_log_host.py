"""CPU-side checks of the episode log (include/mapf_hip.h mapf_set_episode_log, mapf_episode_log): the entry points validate their
arguments before a handle is touched, header / library / ctypes table agree on them and on the record, the ABI and mapf_rollout_io
are what they were, the four new compilations are the Makefile's fourth table (the first three are what they were) and hold exactly
the declared instances without register spills or scratch, the joint units compile to the listings the commit before the log gave
them, the route and the names of launches without the mode are what they were, and policies.episode_statistics agrees with plain
numpy.  No compute is launched here.  (What needs a live handle -- a log without a budget, a log too large, the budget switched off
under a log, graph_begin -- is refused on the GPU in tests/test_gpu_episode_log.py.)"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gym_mapf_amd import _native as nat
from gym_mapf_amd.envs import policies
from host_shim import CSRC, device_listings, kernel_meta
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import AUTO, LG, PACKED, routed_rollout

HEADER = os.path.join(ROOT, 'include', 'mapf_hip.h')
SOURCE = '../csrc_log/mapf_lg_log'
NEW_SYMBOLS = ('mapf_set_episode_log', 'mapf_episode_log')
FORM = 'NS_12EpisodeLimitENS_13EpisodeBudgetENS_10EpisodeLogE'
TABLE, JOINT, PAIRS = 'NS_11TablePolicyE', 'NS_11JointPolicyE', 'NS_13ConflictPairsE'
# per new compilation: {the mangled argument pack behind (args, A): its instances}, and the kernels it holds beside them
PACKS = {'mapf_lg_log_budget': ({FORM: 112, TABLE + FORM: 56}, ('reset_log_partials_kernel',)),
         'mapf_lg_log_pairs_budget': ({FORM + PAIRS: 112, TABLE + FORM + PAIRS: 56}, ()),
         'mapf_lg_log_joint_budget': ({JOINT + FORM: 56}, ()),
         'mapf_lg_log_joint_pairs_budget': ({JOINT + FORM + PAIRS: 56}, ())}
NEW_UNITS = tuple(PACKS)
ADDED_UNITS = ('mapf_lg_pairs_plain', 'mapf_lg_pairs_limit', 'mapf_lg_pairs_budget')
# sha256 of the device listings (hipcc -S --cuda-device-only, __hip_cuid_* masked) of the units that follow a joint table policy, as
# the commit before the episode log compiles them: the units keep their code
PARENT_LISTINGS = {
    'mapf_lg_joint_plain': 'c1335cc35a0c180cb58108fed62bf0fc7ab27dad90a56d5f36b4236421eee8be',
    'mapf_lg_joint_limit': '2f69ee836f9077a17e9d13febc6111e847c4f1dd3cae2f539e346a93ee6ae03f',
    'mapf_lg_joint_budget': 'dea219a089d7d2cb8761814f7b76e1c11494623c184ec1e3d3c8c61393d0e1a7',
    'mapf_lg_joint_pairs_plain': '5ea66437b3a5253ddc6eb8dcdab86de28b7731e354a78ca8766f3ee185422f5c',
    'mapf_lg_joint_pairs_limit': '84b654bc161992c1ee9e51ac7caa7634503b247f1a410e6c02d6a85ff674a24d',
    'mapf_lg_joint_pairs_budget': '8736547573d28d2a6c3491cb2172894be3ffa61e3f0667d242bf9040f4ebd6d6',
}
JOINT_UNITS = tuple(PARENT_LISTINGS)


def test_the_new_entry_points_validate_their_arguments_without_a_device():
    lib = nat.load()
    records, count = np.zeros(4, nat.EPISODE_RECORD_DTYPE), np.zeros(4, np.uint32)
    assert lib.mapf_set_episode_log(None, 3) == nat.MAPF_EINVAL and b'set_episode_log: null handle' in lib.mapf_last_error()
    assert lib.mapf_set_episode_log(None, 0) == nat.MAPF_EINVAL
    assert lib.mapf_episode_log(None, records.ctypes.data, count.ctypes.data, 1) == nat.MAPF_EINVAL and b'episode_log: null handle' in lib.mapf_last_error()
    fake = ctypes.c_void_p(1)                   # (never dereferenced: the pointers are looked at first)
    assert lib.mapf_episode_log(fake, None, None, 0) == nat.MAPF_EINVAL and b'out_records and out_count are null and clear is 0' in lib.mapf_last_error()
    assert not records['outcome'].any() and not count.any()


def test_header_library_and_ctypes_table_agree_on_the_new_names_and_the_record():
    lib = nat.load()
    raw = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\s*\(' % name, text), name
        assert hasattr(lib, name) and name in nat.SIGNATURES, name
        declared = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(declared.split(',')) == len(nat.SIGNATURES[name][1]), name      # one ctypes argument per declared one
    # the record: 16 bytes, the same three fields in the header, the ctypes structure and the numpy dtype
    body = re.search(r'typedef struct mapf_episode_record \{(.*?)\} mapf_episode_record;', text, flags=re.S).group(1)
    fields = [f for f, _ in nat.MapfEpisodeRecord._fields_]
    assert re.findall(r'(\w+);', body) == fields == [f for f, _ in nat.EPISODE_RECORD_DTYPE] == ['ret', 'steps', 'outcome']
    assert ctypes.sizeof(nat.MapfEpisodeRecord) == np.dtype(nat.EPISODE_RECORD_DTYPE).itemsize == 16
    assert [getattr(nat.MapfEpisodeRecord, f).offset for f in fields] == [np.dtype(nat.EPISODE_RECORD_DTYPE).fields[f][1] for f in fields] == [0, 8, 12]
    for bit, (macro, value) in enumerate((('DONE', nat.MAPF_EPISODE_DONE), ('COLLISION', nat.MAPF_EPISODE_COLLISION), ('TRUNCATED', nat.MAPF_EPISODE_TRUNCATED))):
        assert re.search(r'#define\s+MAPF_EPISODE_%s\s+0x%xu' % (macro, 1 << bit), raw) and value == 1 << bit
    # the two "out of scope" sentences no longer list the log; discounting stays out of scope
    assert 'a per-episode log' not in raw and 'per-step or per-episode' not in raw and raw.count('discounting') >= 2
    # new symbols only: the ABI version and the rollout's argument block stay
    assert lib.mapf_abi_version() == nat.MAPF_ABI_VERSION == 6 and re.search(r'#define\s+MAPF_ABI_VERSION\s+6\b', raw)
    fields = [f for f, _ in nat.MapfRolloutIO._fields_]
    body = re.search(r'typedef struct mapf_rollout_io \{(.*?)\} mapf_rollout_io;', text, flags=re.S).group(1)
    assert re.findall(r'(\w+);', body) == fields and fields[-1] == 'rec_prob' and ctypes.sizeof(nat.MapfRolloutIO) == 88


def _table(target):
    text = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, target], universal_newlines=True)
    return dict(line.split() for line in text.splitlines())


def test_the_new_units_are_the_makefiles_fourth_table():
    first, added, joint, log = (_table('print-%skernel-units' % t) for t in ('', 'added-', 'joint-', 'log-'))
    assert log == {unit: SOURCE for unit in NEW_UNITS} and list(log) == list(NEW_UNITS) == list(device_listings.log_units())
    assert os.path.exists(os.path.join(CSRC, SOURCE + '.hip'))
    assert len(first) == 20 and list(added) == list(ADDED_UNITS) and list(joint) == list(JOINT_UNITS) == list(device_listings.joint_units())
    assert set(joint.values()) == {'../csrc_joint/mapf_lg_joint'} and not (set(first) | set(added) | set(joint)) & set(log)
    assert sorted(os.listdir(os.path.join(CSRC, '..', 'csrc_log'))) == ['mapf_lg_log.hip']
    dry = subprocess.check_output(['make', '--no-print-directory', '-C', CSRC, '-n', '-B', 'all', 'listings'], universal_newlines=True)
    for unit in list(first) + list(added) + list(joint) + list(log):
        assert '/%s.o' % unit in dry and '/%s.s' % unit in dry, unit


@pytest.mark.parametrize('unit', NEW_UNITS)
def test_a_new_unit_holds_its_declared_instances_free_of_spills_and_scratch(unit):
    kernels = kernel_meta.kernels(device_listings.listings(unit)[unit])
    packs, others = PACKS[unit]
    source = open(os.path.join(CSRC, SOURCE + '.hip')).read()
    # the family comments declare the counts: 7 group sizes x FULL x MV_LDS x RECORD (x (STREAM | table)), guarded only
    assert re.search(r'each joint unit: 7 group sizes x FULL x MV_LDS x RECORD = 56 instances', source)
    assert re.search(r'each unit without the joint policy: 7 group sizes x FULL x MV_LDS x RECORD x \(STREAM \| table\) = 168 instances', source)
    declared = 56 if 'joint' in unit else 168
    assert sum(packs.values()) == declared == 7 * 2 * 2 * 2 * (1 if 'joint' in unit else 3)
    for pack, want in packs.items():
        got = [k for k in kernels if 'lg_rollout_kernelI' in k['name'] and 'J' + pack + 'EE' in k['name']]
        assert len(got) == want, (unit, pack, len(got))
        assert not any('Lb1EJ' in k['name'] for k in got), unit                     # DENSE, the last flag before the pack: never
    assert len(kernels) == declared + len(others) and all(any(o in k['name'] for k in kernels) for o in others), unit
    assert ('ConflictPairs' in ''.join(k['name'] for k in kernels)) == ('pairs' in unit)
    for k in kernels:
        assert (k['sgpr_spill'], k['vgpr_spill'], k['scratch']) == (0, 0, 0), k


def test_the_joint_units_keep_their_code():
    for unit, want in PARENT_LISTINGS.items():
        text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', device_listings.listings(unit)[unit])
        assert 'EpisodeLog' not in text, unit
        assert hashlib.sha256(text.encode()).hexdigest() == want, unit


def test_the_route_with_the_fact_off_is_what_it_was(shim):
    """tests/host_tables_shim.hip routes with the argument list it had (the `logged` fact defaults to off): the 8-agent bench shape
    under the table policy still takes a packed kernel, and the limit / budget instances their names"""
    for limited, budgeted, want_family, want in ((0, 0, PACKED, 'lq_rollout_kernel_table<'), (1, 0, LG, 'lg_rollout_kernel_table_limit_guarded<'),
                                                 (1, 1, LG, 'lg_rollout_kernel_table_budget_guarded<')):
        family, _, name = routed_rollout(shim, 683, 8, 65536, AUTO, 2, limited=limited, budgeted=budgeted, table_bytes=8 * 683)
        assert family == want_family and name.startswith(want) and 'LOG' not in name and 'log' not in name, name
    _, _, name = routed_rollout(shim, 683, 8, 65536, AUTO, 2, limited=1, budgeted=1, table_bytes=8 * 683)
    assert ',BUDGET>' in name and '; episode budget; table policy:' in name, name      # (the note as it was: no log between the two)


# ------------------------------------------------------------------- envs/policies.py
def test_episode_statistics_against_plain_numpy():
    rs = np.random.RandomState(11)
    E, C = 7, 6
    log = {'episode_returns': rs.randn(E, C) * 3 - 1, 'episode_steps': rs.randint(0, 9, (E, C)).astype(np.uint32),
           'episode_outcomes': rs.choice([1, 3, 4], (E, C)).astype(np.uint8)}
    got = policies.episode_statistics(log)
    per, pooled = got['per_env'], got['pooled']
    r, s, o = log['episode_returns'], log['episode_steps'], log['episode_outcomes']
    assert np.array_equal(per['n'], np.full(E, C)) and pooled['n'] == E * C
    assert np.allclose(per['mean'], r.mean(axis=1)) and np.allclose(per['std'], r.std(axis=1, ddof=1))
    assert np.allclose(per['stderr'], r.std(axis=1, ddof=1) / np.sqrt(C))
    assert np.isclose(pooled['mean'], r.mean()) and np.isclose(pooled['std'], r.std(ddof=1)) and np.isclose(pooled['stderr'], r.std(ddof=1) / np.sqrt(E * C))
    for key, code in (('goal_share', 1), ('collision_share', 3), ('truncated_share', 4)):
        assert np.allclose(per[key], (o == code).mean(axis=1)) and np.isclose(pooled[key], (o == code).mean())
    assert np.allclose(per['goal_share'] + per['collision_share'] + per['truncated_share'], 1.0)
    assert np.allclose(per['mean_steps'], s.mean(axis=1)) and np.array_equal(per['max_steps'], s.max(axis=1))
    assert np.isclose(pooled['mean_steps'], s.mean()) and pooled['max_steps'] == s.max()
    # a log as VecMapfEnv.episode_log returns it: only the first min(count, C) columns of an env are read
    count = np.asarray([6, 2, 9, 1, 0, 3, 6], np.uint32)
    raw = {'returns': r, 'steps': s, 'outcome': o, 'count': count}
    per, pooled = (policies.episode_statistics(raw)[k] for k in ('per_env', 'pooled'))
    n = np.minimum(count, C)
    assert np.array_equal(per['n'], n) and pooled['n'] == n.sum()
    flat = np.concatenate([r[e, :n[e]] for e in range(E)])
    assert np.isclose(pooled['mean'], flat.mean()) and np.isclose(pooled['std'], flat.std(ddof=1))
    for e in range(E):
        if n[e] >= 2:
            assert np.isclose(per['mean'][e], r[e, :n[e]].mean()) and np.isclose(per['std'][e], r[e, :n[e]].std(ddof=1))
            assert per['max_steps'][e] == s[e, :n[e]].max() and np.isclose(per['collision_share'][e], (o[e, :n[e]] == 3).mean())
    assert np.isnan(per['std'][3]) and np.isclose(per['mean'][3], r[3, 0]) and np.isnan(per['mean'][4]) and per['max_steps'][4] == 0
    with pytest.raises(ValueError):
        policies.episode_statistics({'returns': r, 'steps': s[:, :3], 'outcome': o})
