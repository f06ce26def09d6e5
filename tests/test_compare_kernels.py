"""tools/compare_kernels.py, the kernel-by-kernel comparison of two device listings, on tiny hand-written listings: a kernel that was
renamed (a mode's own kernel -> an instance of the template with the mode's argument type) and whose function number and labels
moved passes; one changed instruction, one changed descriptor field, one changed metadata field are each reported; a kernel without a
partner is reported.  No compiler, no device."""
from host_shim import compare_kernels

OLD_LIMIT = '_ZN4mapf20lg_step_kernel_limitILi2ELb1ELb0EEEvNS_8StepArgsEjNS_12EpisodeLimitE'
NEW_LIMIT = '_ZN4mapf14lg_step_kernelILi2ELb1ELb0EJNS_12EpisodeLimitEEEEvNS_8StepArgsEjDpKT2_'
PLAIN = '_ZN4mapf14lg_step_kernelILi2ELb1ELb0EEEvNS_8StepArgsEj'
NEW_PLAIN = '_ZN4mapf14lg_step_kernelILi2ELb1ELb0EJEEEvNS_8StepArgsEjDpKT2_'
HELPER = '_ZN4mapf17reset_ages_kernelEPjPKhm'


def function(symbol, number, tmp, add='v_add_u32_e32 v1, v0, v2', vgpr=3):
    """the text hipcc -S gives a kernel: label, code, the descriptor inside the function, its end"""
    return '''\t.section\t.text.{s},"axG",@progbits,{s},comdat
\t.protected\t{s} ; -- Begin function {s}
\t.globl\t{s}
\t.p2align\t8
\t.type\t{s},@function
{s}: ; @{s}
; %bb.0:
\ts_load_dword s2, s[0:1], 0x108
.Ltmp{t}:
\tv_cmp_gt_u32_e32 vcc, s2, v0
\ts_cbranch_vccz .LBB{n}_2
; %bb.1:
\t{add}
.LBB{n}_2:
.Ltmp{t1}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {s}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_kernarg_size 560
\t\t.amdhsa_next_free_vgpr {v}
\t.end_amdhsa_kernel
\t.section\t.text.{s},"axG",@progbits,{s},comdat
.Lfunc_end{n}:
\t.size\t{s}, .Lfunc_end{n}-{s}
                                        ; -- End function
\t.set {s}.num_vgpr, {v}
'''.format(s=symbol, n=number, t=tmp, t1=tmp + 1, add=add, v=vgpr)


def entry(symbol, vgpr=3, kernarg=560):
    return '''  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           264
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .kernarg_segment_size: {k}
    .name:           {s}
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         {s}.kd
    .vgpr_count:     {v}
    .vgpr_spill_count: 0
'''.format(s=symbol, v=vgpr, k=kernarg)


def listing(functions, entries, cuid='0123abcd'):
    return ('\t.text\n' + ''.join(functions) + '\t.type\t__hip_cuid_%s,@object\n' % cuid
            + '\t.amdgpu_metadata\n---\namdhsa.kernels:\n' + ''.join(entries) + 'amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n')


OLD = listing([function(PLAIN, 0, 0), function(OLD_LIMIT, 1, 2), function(HELPER, 2, 4)], [entry(PLAIN), entry(OLD_LIMIT), entry(HELPER)])


def test_names_of_both_shapes_are_the_same_kernel():
    ck = compare_kernels
    assert ck.parse(NEW_LIMIT) == ('lg_step_kernel', [2, 1, 0], ['EpisodeLimit'])
    assert ck.parse(PLAIN) == ('lg_step_kernel', [2, 1, 0], None) and ck.parse(HELPER) == (None, None, None)
    assert ck.key_of(OLD_LIMIT) == ck.key_of(NEW_LIMIT) == ('lg_step', ('limit',), (2, 1, 0))
    assert ck.key_of(PLAIN) == ck.key_of(NEW_PLAIN) == ('lg_step', (), (2, 1, 0)) != ck.key_of(NEW_LIMIT)
    assert ck.key_of(HELPER) == ('symbol', HELPER)
    # the rollout families: the kernels the modes used to be, and the template's pack
    assert (ck.key_of('_ZN4mapf37lg_rollout_kernel_table_limit_guardedILi4ELb1ELb0ELb1ELb1EEEvNS_11RolloutArgsEjNS_11TablePolicyENS_12EpisodeLimitE')
            == ck.key_of('_ZN4mapf17lg_rollout_kernelILi4ELb1ELb0ELb1ELb0ELb0EJNS_11TablePolicyENS_12EpisodeLimitEEEEvNS_11RolloutArgsEjDpKT5_')
            == ('lg_rollout', ('limit', 'table'), (4, 1, 0, 1, 0, 0)))
    assert (ck.key_of('_ZN4mapf32lg_rollout_kernel_budget_guardedILi4ELb1ELb0ELb1ELb1EEEvNS_11RolloutArgsEjNS_12EpisodeLimitENS_13EpisodeBudgetE')
            == ck.key_of('_ZN4mapf17lg_rollout_kernelILi4ELb1ELb0ELb1ELb1ELb0EJNS_12EpisodeLimitENS_13EpisodeBudgetEEEEvNS_11RolloutArgsEjDpKT5_')
            == ('lg_rollout', ('budget', 'limit'), (4, 1, 0, 1, 1, 0)))
    assert (ck.key_of('_ZN4mapf23lg_rollout_kernel_tableILi4ELb1ELb0ELb1ELb1ELb1EEEvNS_11RolloutArgsEjNS_11TablePolicyE')
            == ck.key_of('_ZN4mapf17lg_rollout_kernelILi4ELb1ELb0ELb1ELb0ELb1EJNS_11TablePolicyEEEEvNS_11RolloutArgsEjDpKT5_')
            == ('lg_rollout', ('table',), (4, 1, 0, 1, 0, 1)))
    assert (ck.key_of('_ZN4mapf12_GLOBAL__N_129lq_rollout_kernel_table_limitILi2ELi4ELb1ELb0ELb0ELb1ELi0ELi2EEEvNS_11RolloutArgsEjjNS_11TablePolicyEjNS_12EpisodeLimitE')
            == ck.key_of('_ZN4mapf12_GLOBAL__N_117lq_rollout_kernelILi2ELi4ELb1ELb0ELb0ELb0ELb1ELi0ELi2EJNS_11TablePolicyEjNS_12EpisodeLimitEEEEvNS_11RolloutArgsEjjDpKT8_')
            == ('lq_rollout', ('limit', 'table'), (2, 4, 1, 0, 0, 0, 1, 0, 2)))
    assert (ck.key_of('_ZN4mapf12_GLOBAL__N_117lq_rollout_kernelILi2ELi4ELb1ELb1ELb0ELb0ELb1ELi0EEEvNS_11RolloutArgsEjj')
            == ck.key_of('_ZN4mapf12_GLOBAL__N_117lq_rollout_kernelILi2ELi4ELb1ELb1ELb0ELb0ELb1ELi0ELi0EJEEEvNS_11RolloutArgsEjjDpKT8_')
            == ('lq_rollout', (), (2, 4, 1, 1, 0, 0, 1, 0, 0)))


def test_a_renamed_kernel_with_the_same_body_passes():
    # other symbols, another order, other function and label numbers, another per-file hash
    new = listing([function(HELPER, 0, 7), function(NEW_LIMIT, 1, 0), function(NEW_PLAIN, 2, 11)], [entry(NEW_LIMIT), entry(HELPER), entry(NEW_PLAIN)],
                  cuid='fedc9876')
    ok, report = compare_kernels.compare(OLD, new, 'tiny')
    assert ok and report == ['same code   tiny  3/3 kernels'], report


def test_one_changed_instruction_descriptor_or_metadata_field_is_reported():
    rest = [function(NEW_PLAIN, 2, 11), function(HELPER, 0, 7)], [entry(NEW_PLAIN), entry(HELPER)]
    for what, changed, e in (('code', function(NEW_LIMIT, 1, 0, add='v_add_u32_e32 v1, v2, v0'), entry(NEW_LIMIT)),
                             ('descriptor', function(NEW_LIMIT, 1, 0, vgpr=4), entry(NEW_LIMIT)),
                             ('meta', function(NEW_LIMIT, 1, 0), entry(NEW_LIMIT, kernarg=568))):
        ok, report = compare_kernels.compare(OLD, listing(rest[0] + [changed], rest[1] + [e]), 'tiny')
        assert not ok and report[0] == 'NOT the same  tiny  2/3 kernels' and len(report) == 2, report
        assert report[1].startswith('DIFFERENT  tiny  %s: %s (%d code lines differ)' % (NEW_LIMIT, what, what == 'code')), report
        assert 'old ' + OLD_LIMIT in report[1] and 'instructions 5 ' in report[1], report


def test_a_kernel_without_a_partner_is_reported():
    # the limit instance is missing on the new side, and another instance (L = 4) has appeared
    other = NEW_LIMIT.replace('ILi2E', 'ILi4E')
    new = listing([function(NEW_PLAIN, 0, 0), function(other, 1, 2), function(HELPER, 2, 4)], [entry(NEW_PLAIN), entry(other), entry(HELPER)])
    ok, report = compare_kernels.compare(OLD, new, 'tiny')
    assert not ok and report[0] == 'NOT the same  tiny  2/3 kernels', report
    assert sorted(line.split()[:4] for line in report[1:]) == [['UNPAIRED', 'tiny', 'new', 'kernel'], ['UNPAIRED', 'tiny', 'old', 'kernel']], report
    assert any(OLD_LIMIT in line for line in report[1:]) and any(other in line for line in report[1:])
    # two kernels of one side that are the same instance: no bijection
    ok, report = compare_kernels.compare(OLD, listing([function(NEW_LIMIT, 0, 0), function(OLD_LIMIT, 1, 2), function(PLAIN, 2, 4), function(HELPER, 3, 6)],
                                                      [entry(NEW_LIMIT), entry(OLD_LIMIT), entry(PLAIN), entry(HELPER)]), 'tiny')
    assert not ok and any(line.startswith('AMBIGUOUS') for line in report), report
