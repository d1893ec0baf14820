"""The gates of the prompt-emphasis kernel tests against the CPU emulation of tests/xattn_keyweight_emul.py (no GPU): the fp64 reference with integer weights is the
unweighted attention over repeated keys, every case's emulated floor sits at or below half of its gate, every deliberate mistake is caught by a case it applies to, and a
table of zeros gives the bits of the plain emulation of tests/attn_emul.py."""
import pytest
import torch

from tests import attn_emul as AE
from tests import kernel_emul as KE
from tests import xattn_keyweight_emul as WE


@pytest.mark.parametrize('size', ['xs', 'xs64'])
@pytest.mark.parametrize('Lk', WE.LKS)
def test_integer_weights_are_repeated_keys_in_fp64(size, Lk):
    c = WE.kw_case(size, 33, Lk, 'g', 'plain', 64)
    b = WE.GROUP.index('int')
    w = c.w[b][c.valid[b]]
    assert bool((w == w.round()).all()) and float(w.max()) > 1
    d = float((c.ref[b] - c.reference_repeated(b)).abs().max())
    print(size, Lk, 'max-abs of the weighted formula from the repeated keys: %.3e' % d)
    assert d < 1e-12, d


@pytest.mark.parametrize('case', WE.KW_CASES + WE.UNIFORM_CASES, ids=WE.case_id)
def test_emulated_floor_is_at_most_half_of_each_gate(case):
    c = WE.kw_case(*case)
    f = c.stats(c.emulated[0])
    g = WE.gates(case)
    own = WE.KW_GATES.get(WE.case_id(case), {})
    print(WE.case_id(case), {k: '%.4e' % f[k] for k in WE.stat_keys(case)}, c.emulated[1])
    assert AE.bitwise_ok(f), f
    for k in WE.stat_keys(case):
        if k in own:
            gate, floor = own[k]
            assert f[k] <= floor * 1.005, (k, f[k], floor)
            assert abs(gate - 2 * floor) <= 0.01 * gate, (k, gate, floor)
            base = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS) if case[4] == 'plain' else dict(a=KE.GATE_XATTN_A, b=KE.GATE_XATTN_B, abs=KE.GATE_XATTN_ABS)
            assert floor > base[k] / 2, (k, floor, base[k])      # a gate of its own only where the shared one is too tight
        else:
            assert f[k] <= g[k] / 2, (k, f[k], g[k])


def test_both_paths_meet_a_bias_and_the_rescale_fires_behind_the_first_tile():
    tot = {}
    for case in WE.KW_CASES:
        for k, v in WE.kw_case(*case).emulated[1].items():
            tot[k] = tot.get(k, 0) + v
    for k in ('full_biased', 'mixed_biased', 'fired_t1'):
        assert tot[k] > 0, (k, tot)


@pytest.mark.parametrize('mut', WE.MUTANTS)
def test_each_deliberate_mistake_is_caught(mut):
    seen = []
    for case in WE.KW_CASES:
        c = WE.kw_case(*case)
        if c.applies(mut) is not None:
            continue
        f = c.stats(c.emul(mut)[0])
        seen.append((WE.case_id(case), WE.caught(f, WE.gates(case))))
    assert seen, 'the mistake applies to no case'
    assert any(ok for _, ok in seen), seen


@pytest.mark.parametrize('case', WE.UNIFORM_CASES + [c for c in WE.KW_CASES if c[4] == 'plain'], ids=WE.case_id)
def test_zero_bias_is_the_plain_emulation_bit_for_bit(case):
    """uniform weights (every weight 3.0: a table of zeros) through the emphasis emulation, full and mixed path, against tests/attn_emul.py's on the same buffers.  On the
    grouped cases the weights are replaced by a uniform row first."""
    c = WE.kw_case(*case)
    if case[3] != WE.UNIFORM:
        c = WE.KeyWeightCase(*case)
        c.w = torch.where(c.valid, torch.full_like(c.w, 3.0), c.w)
    assert not bool(WE.bias_table(c.w, c.valid, c.Lkp).any())
    assert c.emulated[1]['full'] > 0 and c.emulated[1]['mixed'] > 0
    assert torch.equal(c.emulated[0], c.plain_twin().emul()[0])


def test_the_bias_table_is_what_the_setter_documents():
    c = WE.kw_case('xs', 130, 384, 'g', 'plain', 64)
    bias = WE.bias_table(c.w, c.valid, c.Lkp)
    assert bool(torch.isfinite(bias).all()) and bool((bias <= 0).all())
    assert bool((bias[~c.valid] == 0).all())
    assert bool((bias.max(1).values == 0).all())
    pk, wd = WE.GROUP.index('peak'), WE.GROUP.index('wide')
    assert sorted(set(bias[pk][c.valid[pk]].tolist())) == [-20.0, 0.0]
    assert sorted(set(bias[wd][c.valid[wd]].tolist())) == [-20.0, 0.0]
    one = WE.kw_case('xs', 130, 100, 'g', 'plain', 64)      # the single-key row: its one key at 2^-20 is a bias of 0
    assert int(one.valid[wd].sum()) == 1 and not bool(WE.bias_table(one.w, one.valid, one.Lkp)[wd].any())
