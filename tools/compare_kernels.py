#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two hipcc -S device listings of one unit, for a change that renames or merges kernels: the
listings then differ byte for byte (tools/compare_device_listings.sh) although every instance compiled to the code it had.

    python tools/compare_kernels.py OLD.s NEW.s [unit name]      (exit 0 = every kernel paired, every pair the same)

Pairing: a kernel is (family, modes, template arguments), read from its mangled name (no demangler is needed: the names are of the
few shapes parse() knows); RULES says what each kernel name of the lane-group and packed rollout / step families means -- the
eleven names they had as separate kernels, and the three templates whose modes are the types of their trailing argument pack.
Any other kernel pairs by its symbol.  The pairing must be a bijection.
Code: a pair's text from its label to its .amdhsa_kernel descriptor, with the kernel's own symbol, the function's number in
.LBB<n>_ / .LJTI<n>_ labels, the numbering of .Ltmp<n> labels (renumbered by first appearance) and __hip_cuid_* masked.
Resources: a pair's .amdhsa_kernel descriptor and its .amdgpu_metadata entry, with the symbol masked.

Prints `same code  <unit>  N/N kernels`, or the kernels without a partner and the pairs that differ, with their line counts and
registers on both sides."""
import re
import sys

TABLE, LIMIT, BUDGET, JOINT = 'table', 'limit', 'budget', 'joint'
PACK_MODES = {'TablePolicy': TABLE, 'EpisodeLimit': LIMIT, 'EpisodeBudget': BUDGET, 'JointPolicy': JOINT}


def parse(symbol):
    """(kernel name, [template argument values], [type names of a trailing pack] or None); (None, None, None) for a name that is
    no template instance of namespace mapf"""
    m = re.match(r'_ZN4mapf(?:12_GLOBAL__N_1)?(\d+)', symbol)
    if not m:
        return None, None, None
    at = m.end() + int(m.group(1))
    name, rest = symbol[m.end():at], symbol[at:]
    if not rest.startswith('I'):
        return None, None, None
    rest, values, pack = rest[1:], [], None
    while not rest.startswith('E'):
        lit = re.match(r'L[ibj](\d+)E', rest)
        if lit and pack is None:
            values.append(int(lit.group(1)))
            rest = rest[lit.end():]
        elif rest.startswith('J') and pack is None:           # the argument pack: class types of the namespace, or builtin ones
            rest, pack = rest[1:], []
            while not rest.startswith('E'):
                t = re.match(r'NS_(\d+)', rest)
                if t:
                    end = t.end() + int(t.group(1))
                    pack.append(rest[t.end():end])
                    assert rest[end] == 'E', symbol
                    rest = rest[end + 1:]
                else:
                    assert rest[0] in 'jimy', symbol
                    pack.append(rest[0])
                    rest = rest[1:]
            rest = rest[1:]
        else:
            raise ValueError('template arguments of %s' % symbol)
    return name, values, pack


def _modes(pack):
    return tuple(sorted(PACK_MODES[t] for t in pack or () if t in PACK_MODES))


# kernel name -> (family, what (values, pack) mean: (modes, canonical template arguments))
#   lg_rollout: (L, FULL, MV_LDS, RECORD, STREAM, DENSE); lg_step: (L, FULL, EXT_UNIFORMS);
#   lq_rollout: (Q, K, RECORD, STREAM, SOC, COMPACT, TERM, BITMAP, TABLE)
RULES = {
    # the templates (and, with no pack, the plain kernels as they were)
    'lg_rollout_kernel': ('lg_rollout', lambda v, p: (_modes(p), tuple(v))),
    'lg_step_kernel': ('lg_step', lambda v, p: (_modes(p), tuple(v))),
    'lq_rollout_kernel': ('lq_rollout', lambda v, p: (_modes(p), tuple(v) + ((0,) if len(v) == 8 else ()))),
    # the kernels the modes used to be: <L, FULL, MV_LDS, RECORD, DENSE, TABLE>, <..., RECORD, STREAM>, <..., RECORD, TABLE>
    'lg_rollout_kernel_table': ('lg_rollout', lambda v, p: ((TABLE,), (v[0], v[1], v[2], v[3], 0, v[4]))),
    'lg_rollout_kernel_limit_guarded': ('lg_rollout', lambda v, p: ((LIMIT,), (v[0], v[1], v[2], v[3], v[4], 0))),
    'lg_rollout_kernel_table_limit_guarded': ('lg_rollout', lambda v, p: ((LIMIT, TABLE), (v[0], v[1], v[2], v[3], 0, 0))),
    'lg_rollout_kernel_budget_guarded': ('lg_rollout', lambda v, p: ((BUDGET, LIMIT), (v[0], v[1], v[2], v[3], v[4], 0))),
    'lg_rollout_kernel_table_budget_guarded': ('lg_rollout', lambda v, p: ((BUDGET, LIMIT, TABLE), (v[0], v[1], v[2], v[3], 0, 0))),
    'lg_step_kernel_limit': ('lg_step', lambda v, p: ((LIMIT,), tuple(v))),
    # <Q, K, RECORD, SOC, COMPACT, TERM, BITMAP, TABLE>: no STREAM
    'lq_rollout_kernel_table': ('lq_rollout', lambda v, p: ((TABLE,), (v[0], v[1], v[2], 0) + tuple(v[3:]))),
    'lq_rollout_kernel_table_limit': ('lq_rollout', lambda v, p: ((LIMIT, TABLE), (v[0], v[1], v[2], 0) + tuple(v[3:]))),
}


def key_of(symbol):
    """what a kernel is, whatever it is called"""
    name, values, pack = parse(symbol)
    if name not in RULES:
        return ('symbol', symbol)
    family, rule = RULES[name]
    return (family,) + rule(values, pack)


def split(text):
    """{symbol: dict(code=[lines], descriptor=[lines], meta=[lines])} of a listing, everything masked"""
    text = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', text)
    lines = text.split('\n')
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r'(\S+):\s+; @(\S+)$', line)
        if not m or m.group(1) != m.group(2) or i == 0 or not re.match(r'\s+\.type\s+%s,@function' % re.escape(m.group(1)), lines[i - 1]):
            continue
        symbol = m.group(1)
        d = next(j for j in range(i, len(lines)) if lines[j].strip() == '.amdhsa_kernel ' + symbol)
        end = next(j for j in range(d, len(lines)) if lines[j].strip() == '.end_amdhsa_kernel')
        assert re.match(r'\.Lfunc_end\d+:', lines[end + 2]), (symbol, lines[end + 2])   # (the descriptor sits inside the function's text)
        tmp = {}
        def mask(s):
            s = s.replace(symbol, '<kernel>')
            s = re.sub(r'\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+', r'.\1N', s)
            return re.sub(r'\.Ltmp\d+', lambda t: tmp.setdefault(t.group(0), '.Ltmp#%d' % len(tmp)), s)
        out[symbol] = dict(code=[mask(s) for s in lines[i:d]], descriptor=[mask(s) for s in lines[d:end + 1]], meta=[])
    for blk in re.split(r'\n  - \.agpr_count:', text)[1:]:
        entry = []
        for s in ('  - .agpr_count:' + blk).split('\n'):
            if s and not s.startswith('  '):                      # the end of the kernels' list
                break
            entry.append(s)
        symbol = re.search(r'\.name:\s+(\S+)', blk).group(1)
        out[symbol]['meta'] = [s.replace(symbol, '<kernel>') for s in entry]
    assert all(k['meta'] for k in out.values()), 'a kernel without a metadata entry'
    return out


def _resources(k):
    f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, '\n'.join(k['meta'])).group(1))
    n_inst = sum(1 for s in k['code'] if re.match(r'\t[a-z]\w+', s))
    return 'vgpr %d sgpr %d lds %d scratch %d instructions %d lines %d' % (f('vgpr_count'), f('sgpr_count'), f('group_segment_fixed_size'),
                                                                         f('private_segment_fixed_size'), n_inst, len(k['code']))


def compare(old_text, new_text, unit='unit'):
    """(ok, report lines)"""
    old, new = split(old_text), split(new_text)
    by_key = [{}, {}]
    report = []
    for side, kernels in enumerate((old, new)):
        for symbol in kernels:
            key = key_of(symbol)
            if key in by_key[side]:
                report.append('AMBIGUOUS  %s  %s and %s are both %r' % (unit, by_key[side][key], symbol, key))
            by_key[side][key] = symbol
    for side, tag in ((0, 'old'), (1, 'new')):
        for key, symbol in by_key[side].items():
            if key not in by_key[1 - side]:
                report.append('UNPAIRED   %s  %s kernel %s  %r' % (unit, tag, symbol, key))
    pairs = [(by_key[0][key], by_key[1][key]) for key in by_key[0] if key in by_key[1]]
    same = 0
    for a, b in pairs:
        what = [part for part in ('code', 'descriptor', 'meta') if old[a][part] != new[b][part]]
        if not what:
            same += 1
            continue
        n_diff = sum(1 for x, y in zip(old[a]['code'], new[b]['code']) if x != y) + abs(len(old[a]['code']) - len(new[b]['code']))
        report.append('DIFFERENT  %s  %s: %s (%d code lines differ)\n    old %s  %s\n    new %s  %s'
                      % (unit, b, ', '.join(what), n_diff, a, _resources(old[a]), b, _resources(new[b])))
    ok = not report and len(old) == len(new) == len(pairs)
    head = '%s  %s  %d/%d kernels' % ('same code ' if ok else 'NOT the same', unit, same, max(len(old), len(new)))
    return ok, [head] + report


if __name__ == '__main__':
    ok, report = compare(open(sys.argv[1]).read(), open(sys.argv[2]).read(), sys.argv[3] if len(sys.argv) > 3 else sys.argv[2])
    print('\n'.join(report))
    sys.exit(0 if ok else 1)
