"""The plan of an env.P[s][a] call: plan_transitions and transitions_kernel_name (csrc/mapf_plan.hip) against what the launchers
of the commit before them launched.

tests/golden/transitions_plans.json holds, per shape (agents, queries, window, compacted or reserved rows, all five outputs given or
not), what that commit's launch_transitions handed to the runtime: the return code, the noted name and every launch -- kernel
instance, grid, block, dynamic LDS bytes, the kernel's scalar arguments.  Full rows for the boundary shapes, a SHA-256 per (agents,
layout, outputs) group for the dense sweep.  Recorded without a device by tools/record_transitions_launches.cpp
(generation_info.json says how):

    python tests/test_transitions_plan.py --record RECORDER_BINARY [OUT.json]

A call that is refused is recorded as its return code alone: the old launchers had by then noted a name or launched the scan, the
planner declines before anything is launched."""
import hashlib
import json
import os
import re
import subprocess
import sys

from conftest import GOLDEN
from host_shim import shim  # noqa: F401  (the host shim, built once per run)
from plan_sweeps import KERNEL_NAME_BYTES, declare, planned

FIXTURE = os.path.join(GOLDEN, 'transitions_plans.json')
AGENTS = range(1, 17)
# both sides of every threshold of the arithmetic: the scan block (256) and the fused scan (256 blocks); the wave supply rule
# (16384 waves of 8, 16, 32 queries); the piece sizes at 8 agents and a full window (est. rows / 2048 >= 24576, / 4096 likewise)
BOUNDARY_QUERIES = (1, 255, 256, 257, 65536, 65537, 131071, 131072, 262143, 262144, 524287, 524288, 38356, 38357, 76713, 76714)
BOUNDARY_QUERIES_ACROSS_WINDOWS = (1, 65537)                            # one query; just beyond the fused scan


def boundary_windows(A):
    return (1, 63, 64, 65, 1023, 1025, 3 ** A, 2 ** 24 + 1)


SWEEP_QUERIES = tuple(sorted(set(BOUNDARY_QUERIES) | {2 ** k + d for k in (6, 8, 14, 15, 16, 20, 24) for d in (-1, 0, 1)} |
                             {2, 2000, 20000, 200000, 2 ** 31, 2 ** 37 - 1, 2 ** 37, 2 ** 39, 2 ** 39 + 1, 2 ** 45}))
SWEEP_WINDOWS = (1, 2, 3, 8, 9, 10, 27, 63, 64, 65, 80, 81, 82, 300, 728, 729, 730, 1023, 1024, 1025, 2048, 2049, 2187, 3000, 4096, 6560, 6561, 6562, 19683, 2 ** 20, 2 ** 20 + 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1024)   # (beyond, the wide family's 32-bit chunk arithmetic wraps: not pinned)


def sweep_windows(A):
    return tuple(sorted(set(SWEEP_WINDOWS) | {3 ** A}))


def boundary_shapes():
    """The shapes stored as full rows, 32 per (agents, layout): every boundary query count at the full window; every boundary window at
    two query counts; an output array missing at those two.  (Their whole cross product, with and without all outputs, is part of the
    sweep and so of its digests: full rows are what a failure is read from, the digests what nothing escapes.)"""
    for A in AGENTS:
        for compact in (0, 1):
            for N in BOUNDARY_QUERIES:
                yield A, N, 3 ** A, compact, 1
            for N in BOUNDARY_QUERIES_ACROSS_WINDOWS:
                for M in boundary_windows(A):
                    if M != 3 ** A:
                        yield A, N, M, compact, 1
                yield A, N, 3 ** A, compact, 0


def sweep_groups():
    for A in AGENTS:
        for compact in (0, 1):
            for all_out in (0, 1):
                yield 'A=%d %s %s' % (A, 'compacted' if compact else 'reserved', 'all_out' if all_out else 'some_out'), \
                    [(A, N, M, compact, all_out) for N in SWEEP_QUERIES for M in sweep_windows(A)]


def key_of(shape):
    return '%d %d %d %d %d' % shape


# ---------------------------------------------------------------- one row per shape, from the recorder's line or from the plan
_SHAPE = r'g=(\d+),1,1 b=(\d+),1,1 lds=(\d+)'
_LINE = re.compile(r'rc=0;name=(?P<name>[^;]*)(?:;count %s rel=1 base=1)?(?:;totals g=1,1,1 b=1024,1,1 lds=0 base=1 n=(?P<tn>\d+) total=(?P<tt>[01]))?'
                   r';(?P<kind>rows|wide)<(?P<n>\d+),(?P<flag>[01])> %s (?P<args>[\d ]+)$' % (_SHAPE, _SHAPE))


def row_of_line(line):
    """the recorder's line in the fixture's form; anything the form leaves out must have the one value it can have"""
    if not line.startswith('rc=0;'):
        assert re.match(r'rc=1;name=[^;]*(;count [^;]*)?(;totals [^;]*)?$', line), line
        return 'rc=1', ''
    m = _LINE.match(line)
    assert m, line
    count_grid, count_block, count_lds, grid, block, lds = m.group(2, 3, 4, 10, 11, 12)
    scan = ''
    if count_grid is not None:
        assert (count_block, count_lds) == ('256', '0'), line
        scan = 'c%s' % count_grid
        if m.group('tn') is not None:
            assert m.group('tn') == count_grid, line
            scan += 't%s' % m.group('tt')
    else:
        assert m.group('tn') is None, line
    return '%s|%s<%s,%s> %s %s %s %s' % (scan, m.group('kind'), m.group('n'), m.group('flag'), grid, block, lds, m.group('args')), m.group('name')


def row_of_plan(plan, compact):
    """the launches the dispatcher and the launchers make of a plan, in the fixture's form"""
    if plan is None:
        return 'rc=1'
    scan = ''
    if plan['scan_passes']:
        scan = 'c%d' % plan['scan_blocks'] + ('t%d' % compact if plan['scan_passes'] == 2 else '')
    if plan['wide']:
        kernel = 'wide<%d,1> %d %d %d %d %d %d' % (plan['max_a'], plan['grid'], plan['block'], plan['lds_bytes'], plan['lanes_log2'], plan['chunk'], plan['chunks_per_query'])
    else:
        kernel = 'rows<%d,%d> %d %d %d %d %d %d %d' % (plan['max_a'], plan['all_out'], plan['grid'], plan['block'], plan['lds_bytes'], plan['qw_log2'], plan['pieces_max'],
                                                      plan['rows_per_wave'], plan['unscanned_blocks'])
    return scan + '|' + kernel


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------- the tests
def test_boundary_shapes_plan_what_the_old_launchers_launched(shim):  # noqa: F811
    lib, recorded = declare(shim), _fixture()
    rows, names = recorded['boundary'], recorded['names']
    shapes = list(boundary_shapes())
    assert len(shapes) == len(rows) == 16 * 2 * (16 + 2 * 7 + 2)
    wrong, seen = [], set()
    for shape in shapes:
        plan, name = planned(lib, shape)
        want = rows[key_of(shape)]
        if want == 'rc=1':
            got = row_of_plan(plan, shape[3])
        else:
            idx, want = want.split('|', 1)
            got, want = (row_of_plan(plan, shape[3]), name), (want, names[int(idx)])
            seen.add(want[0].split('|')[1].split(' ')[0])
        if got != want:
            wrong.append((shape, got, want))
    assert not wrong, '%d of %d shapes are planned differently: %s' % (len(wrong), len(shapes), wrong[:6])
    # every instance of both families is among them
    assert set(BOUNDARY_QUERIES) <= set(SWEEP_QUERIES) and all(set(boundary_windows(A)) <= set(sweep_windows(A)) for A in AGENTS)   # the cross product: in the sweep
    assert seen == {'rows<%d,%d>' % (n, o) for n in (2, 4, 6, 8) for o in (0, 1)} | {'wide<%d,1>' % n for n in range(9, 17)}


def test_dense_sweep_digests_and_invariants(shim):  # noqa: F811
    lib, recorded = declare(shim), _fixture()
    digests = recorded['sweep']
    n, n_declined, n_pieces, sizes = 0, 0, 0, set()
    for group, shapes in sweep_groups():
        h = hashlib.sha256()
        for shape in shapes:
            A, N, M, compact, all_out = shape
            plan, name = planned(lib, shape)
            h.update((key_of(shape) + '|' + row_of_plan(plan, compact) + '|' + (name or '') + '\n').encode())
            n += 1
            blocks = lib.shim_transitions_scan_blocks(N)
            assert blocks == (N + 255) // 256
            if plan is None:
                n_declined += 1
                continue
            assert len(name) < KERNEL_NAME_BYTES and plan['grid'] <= 2 ** 31 - 1
            assert plan['scan_blocks'] == (blocks if plan['scan_passes'] else 0)
            if plan['wide']:
                assert A > 8 and plan['max_a'] == A and plan['lds_bytes'] == 0 and plan['block'] == 256
                assert plan['chunk'] == plan['walks'] << plan['lanes_log2'] and plan['chunks_per_query'] * plan['chunk'] >= M > (plan['chunks_per_query'] - 1) * plan['chunk']
                threads = N * plan['chunks_per_query'] << plan['lanes_log2']
                if threads < 2 ** 64:      # (beyond, the 64-bit product wraps as it did before the plan: the digest pins it, nothing here blesses it)
                    assert plan['grid'] == -(-threads // 256)
                assert plan['scan_passes'] == (2 if compact else 0)       # the wide kernels read the scanned totals whenever rows are compacted
                continue
            assert A <= plan['max_a'] < A + 2 and plan['all_out'] == all_out
            waves_per_block = plan['block'] // 64
            assert waves_per_block == (1 if plan['max_a'] >= 6 else 4) and plan['block'] == 64 * waves_per_block
            assert plan['lds_bytes'] == waves_per_block * lib.shim_transitions_wave_lds_bytes(plan['max_a'], plan['qw_log2']) <= 64 * 1024
            waves = -(-N // (1 << plan['qw_log2'])) * plan['pieces_max']
            assert plan['grid'] == -(-waves // waves_per_block)           # the grid covers every (batch, piece) wave
            assert 2 <= plan['qw_log2'] <= 6 and plan['rows_per_wave'] in (1024, 2048, 4096) and plan['pieces_max'] >= 1
            assert plan['pieces_max'] == 1 or (plan['max_a'] >= 6 and plan['pieces_max'] * plan['rows_per_wave'] >= (min(3 ** A, M) << plan['qw_log2']))
            assert (plan['scan_passes'] >= 1) == bool(compact or plan['pieces_max'] > 1)
            if plan['scan_passes']:
                assert (plan['scan_passes'] == 2) == (blocks > 256)       # beyond 256 scan blocks the second pass runs, below the rows kernel adds up
            assert plan['unscanned_blocks'] == (blocks if blocks <= 256 else 0)
            n_pieces += plan['pieces_max'] > 1
            sizes.add(plan['rows_per_wave'])
        assert h.hexdigest() == digests[group], group
    assert n == sum(len(s) for _, s in sweep_groups()) and len(digests) == 64
    assert n_declined > 0 and n_pieces > 0 and sizes == {1024, 2048, 4096}, (n_declined, n_pieces, sizes)


def test_declined_exactly_where_a_grid_overflows(shim):  # noqa: F811
    """false comes back for more than 16 agents and where the launch's grid, or the count pass's when it runs, exceeds 2^31 - 1 blocks --
    stated from the plan's own fields at a shape the planner accepts next to it"""
    lib = declare(shim)
    for compact in (0, 1):
        for A in (17, 18, 128):
            assert planned(lib, (A, 1, 81, compact, 1)) == (None, None)
        # rows, whole windows: a block takes block / 64 waves of 2^qw_log2 queries (at most 256 in all, so the scan's grid is no larger)
        # wide: one group of 64 lanes per query at a window of 64 rows, four groups a block
        for A, M in ((2, 9), (4, 81), (9, 64)):
            plan = planned(lib, (A, 2 ** 30, M, compact, 1))[0]
            per_block = 4 if plan['wide'] else (plan['block'] // 64) << plan['qw_log2']
            assert per_block <= 256 and plan['grid'] == 2 ** 30 // per_block
            assert planned(lib, (A, (2 ** 31 - 1) * per_block, M, compact, 1))[0]['grid'] == 2 ** 31 - 1
            assert planned(lib, (A, (2 ** 31 - 1) * per_block + 1, M, compact, 1)) == (None, None)
    # 8 agents in pieces, one wave a block: the last batch count whose pieces still fit the grid, and one query more
    plan = planned(lib, (8, 2 ** 30, 6561, 0, 1))[0]
    pieces, per_wave = plan['pieces_max'], 1 << plan['qw_log2']
    assert pieces > 1 and plan['block'] == 64 and plan['grid'] == 2 ** 30 // per_wave * pieces
    batches = (2 ** 31 - 1) // pieces
    assert planned(lib, (8, per_wave * batches, 6561, 0, 1))[0]['grid'] == batches * pieces
    assert planned(lib, (8, per_wave * batches + 1, 6561, 0, 1)) == (None, None)


# ---------------------------------------------------------------- recording
def record(recorder, out_path):
    def run(shapes):
        text = ''.join(key_of(s) + '\n' for s in shapes)
        lines = subprocess.run([recorder], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
        assert len(lines) == len(shapes)
        return [row_of_line(line) for line in lines]

    names, boundary = [], {}
    shapes = list(boundary_shapes())
    for shape, (row, name) in zip(shapes, run(shapes)):
        if row == 'rc=1':
            boundary[key_of(shape)] = row
            continue
        if name not in names:
            names.append(name)
        boundary[key_of(shape)] = '%d|%s' % (names.index(name), row)
    sweep = {}
    for group, shapes in sweep_groups():
        h = hashlib.sha256()
        for shape, (row, name) in zip(shapes, run(shapes)):
            h.update((key_of(shape) + '|' + row + '|' + name + '\n').encode())
        sweep[group] = h.hexdigest()
    with open(out_path, 'w') as f:
        json.dump({'names': names, 'boundary': boundary, 'sweep': sweep}, f, indent=0, sort_keys=True)
        f.write('\n')
    print('%d boundary rows, %d names, %d sweep groups of %d shapes in all -> %s' % (len(boundary), len(names), len(sweep), sum(len(s) for _, s in sweep_groups()), out_path))


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == '--record':
        record(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else FIXTURE)
    else:
        sys.exit(__doc__)
