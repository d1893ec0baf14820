"""The gates of the prompt-timeline kernel tests against the CPU emulation of tests/xattn_timeline_emul.py (no GPU): every case's emulated floor sits at or below half of
its gate, every deliberate mistake is caught by a case it applies to, the two halves of the paired mistake and the range-widening mistake change no bit, and a prompt that is
weighted alone gives the bits of the plain emulation on its keys."""
import pytest
import torch

from tests import attn_emul as AE
from tests import xattn_timeline_emul as TE


@pytest.mark.parametrize('case', TE.TL_CASES + TE.ONES_CASES, ids=TE.case_id)
def test_emulated_floor_is_at_most_half_of_each_gate(case):
    c = TE.tl_case(*case)
    f = c.stats(c.emulated[0])
    g = TE.gates(case)
    own = TE.TL_GATES.get(TE.case_id(case), {})
    print(TE.case_id(case), {k: '%.4e' % f[k] for k in TE.stat_keys(case)}, c.emulated[1])
    assert AE.bitwise_ok(f), f
    for k in TE.stat_keys(case):
        if k in own:
            gate, floor = own[k]
            assert f[k] <= floor * 1.005, (k, f[k], floor)
            assert abs(gate - 2 * floor) <= 0.01 * gate, (k, gate, floor)
            base = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS) if case[3] == 'plain' else dict(a=TE.KE.GATE_XATTN_A, b=TE.KE.GATE_XATTN_B, abs=TE.KE.GATE_XATTN_ABS)
            assert floor > base[k] / 2, (k, floor, base[k])      # a gate of its own only where the shared one is too tight
        else:
            assert f[k] <= g[k] / 2, (k, f[k], g[k])


def test_every_path_of_the_timeline_is_walked_by_some_case():
    tot = {}
    for case in TE.TL_CASES:
        for k, v in TE.tl_case(*case).emulated[1].items():
            tot[k] = tot.get(k, 0) + v
    for k in ('skipped', 'full', 'mixed', 'sentinel_rows', 'empty_partners', 't_lo_pos', 't_hi_short', 'fired_t1'):
        assert tot[k] > 0, (k, tot)


@pytest.mark.parametrize('mut', TE.MUTANTS)
def test_each_deliberate_mistake_is_caught(mut):
    seen = []
    for case in TE.TL_CASES:
        c = TE.tl_case(*case)
        if c.applies(mut) is not None:
            continue
        f = c.stats(c.emul(mut)[0])
        seen.append((TE.case_id(case), TE.caught(f, TE.gates(case))))
    assert seen, 'the mistake applies to no case'
    assert any(ok for _, ok in seen), seen


@pytest.mark.parametrize('half', TE.HALF_MUTANTS)
def test_each_half_of_the_paired_mistake_changes_no_bit(half):
    n = 0
    for case in TE.TL_CASES:
        c = TE.tl_case(*case)
        if c.applies('zero_through_exponent_and_empty_partner_weight_one') is not None:
            continue
        assert torch.equal(c.emul(half)[0], c.emulated[0]), (half, TE.case_id(case))
        n += 1
    assert n > 0


def test_padding_queries_that_widen_the_range_cost_tiles_and_change_no_bit():
    n = 0
    for case in TE.TL_CASES:
        c = TE.tl_case(*case)
        if c.applies(TE.RANGE_MUTANT) is not None:
            continue
        buf, counts = c.emul(TE.RANGE_MUTANT)
        assert counts['walked'] > c.emulated[1]['walked'], TE.case_id(case)
        assert torch.equal(buf, c.emulated[0]), TE.case_id(case)
        n += 1
    assert n > 0


@pytest.mark.parametrize('size', ['xs', 'xs64'])
@pytest.mark.parametrize('Lq', TE.LQS)
def test_one_weighted_prompt_is_the_plain_emulation_on_its_keys(size, Lq):
    c = TE.tl_case(size, Lq, 'b', 'plain', 64)
    b = TE.GROUPS['b'].index('one')
    plain = c.plain_on_prompt(1, b).emul()[0]
    assert torch.equal(plain[:Lq], c.emulated[0][b * Lq:(b + 1) * Lq])
    t_lo, t_hi = c._ranges(None)
    assert bool((t_lo[b][:(Lq + 31) // 32] == 1).all()) and bool((t_hi[b][:(Lq + 31) // 32] == 2).all())


def test_the_bias_table_holds_zero_for_the_dominant_prompt_and_off_for_weight_zero():
    w = TE.tl_case('xs', 130, 'b', 'plain', 64).w
    bias, sup = TE.bias_table(w)
    assert bool((bias.max(1).values == 0).all())
    assert bool(((bias == TE.OFF) == (w == 0)).all())
    tiny = TE.GROUPS['b'].index('tiny')
    assert float(bias[tiny, 1, 0]) == -20.0 and float(bias[tiny, 1, TE.TINY_FRAME]) == 0.0 and bool(bias[tiny, 0, TE.TINY_FRAME] == TE.OFF)
    gap = TE.GROUPS['b'].index('gap')
    assert sup[gap].tolist() == [[0, 130], [0, 0], [0, 130]]
    sw = TE.tl_case('xs', 130, 'a', 'plain', 64)
    assert TE.bias_table(sw.w)[1][0].tolist() == [[0, 70], [70, 100], [100, 130]]
