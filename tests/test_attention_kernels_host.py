"""CPU side of the kernel-level tests of plain self-attention (tests/test_attention_kernels_gpu.py): the gates of tests/attn_emul.py against its fp32 emulation and its
deliberate mistakes, the coverage the cases give the deferred rescale, and the refusals of ezdit_test_attention / ezdit_test_attention_varlen that come before the first HIP
call."""
import functools

import pytest
import torch

from tests import attn_emul as AE


@functools.lru_cache(maxsize=None)
def _floor(t):
    c = AE.attn_case(*t)
    buf, counts = c.emulated
    return c.figures(buf), counts


@pytest.mark.parametrize('case', AE.ATTN_CASES, ids=AE.case_id)
def test_emulation_is_clean_and_under_half_of_every_gate(case):
    """per case: the emulation breaks no bitwise check (finite, zeros behind klen[b], the prefill in the columns [D, ldD) and in the rows behind B Lq) and each gated statistic
    is at most its recorded floor, which is at most half its gate"""
    f, _ = _floor(case)
    print(AE.case_id(case), f)
    assert AE.bitwise_ok(f), f
    assert f['head'] <= AE.FLOOR_HEAD * 1.005 and f['row'] <= AE.FLOOR_ROW * 1.005 and f['abs'] <= AE.FLOOR_ABS * 1.005, f
    assert AE.within_gates(f)


def test_gates_are_twice_the_worst_floor_and_not_above_the_older_tests():
    worst = {k: max(_floor(t)[0][k] for t in AE.ATTN_CASES) for k in ('head', 'row', 'abs')}
    print('worst emulated floors:', worst)
    for k, floor, gate, old in (('head', AE.FLOOR_HEAD, AE.GATE_HEAD, AE.OLD_REL), ('row', AE.FLOOR_ROW, AE.GATE_ROW, AE.OLD_REL), ('abs', AE.FLOOR_ABS, AE.GATE_ABS, AE.OLD_ABS)):
        assert 0.98 * floor <= worst[k] <= floor * 1.005, (k, worst[k], floor)      # the recorded floor IS the worst over the cases
        assert 1.9 * floor <= gate <= 2 * floor and gate <= old, (k, floor, gate)


def test_the_deferred_rescale_fires_and_is_deferred_beyond_the_first_tile_in_every_sub_block():
    """the cases reach, for each NKH: a rescale that fires at t >= 1 because of a real query row, one that is deferred there with some P > 1, and both in a sub-block kh >= 1"""
    for nkh in (2, 4):
        for key in ('fired_t1', 'fired_t1_kh1', 'deferred_t1', 'deferred_t1_kh1'):
            best = max(_floor(t)[1][key] for t in AE.ATTN_CASES if t[4] == nkh)
            print(f'nkh {nkh} {key}: {best} events in the best case')
            assert best > 0, (nkh, key)
    # the staircase head alone gives all of it where a sub-block sees three tiles
    for t in AE.ATTN_CASES:
        if t[2] == 385:
            assert all(v > 0 for v in _floor(t)[1].values()), (t, _floor(t)[1])


@functools.lru_cache(maxsize=None)
def _mistake(t, mut):
    c = AE.attn_case(*t)
    return c.figures(c.emul(mut)[0])


def test_every_mistake_is_caught_at_three_times_a_gate_or_by_a_bitwise_check():
    """every mistake of MUTANTS, in at least one case of EACH key-tile size it can be made at (AttnCase.applies names the cases it cannot be made in), breaks a bitwise check
    or puts a gated statistic at three times its gate; and in most of the cases it applies to"""
    for mut in AE.MUTANTS:
        for nkh in (2, 4):
            made = [t for t in AE.ATTN_CASES if t[4] == nkh and AE.attn_case(*t).applies(mut) is None]
            hit = [t for t in made if AE.caught(_mistake(t, mut))]
            skipped = {AE.case_id(t): AE.attn_case(*t).applies(mut) for t in AE.ATTN_CASES if t[4] == nkh and AE.attn_case(*t).applies(mut)}
            print(f'{mut} nkh {nkh}: caught in {len(hit)} of {len(made)} cases; not made in {skipped}')
            assert made and hit, (mut, nkh)
            assert len(hit) >= 0.9 * len(made), (mut, nkh, [AE.case_id(t) for t in made if t not in hit])


def test_every_mistake_is_made_in_a_fair_number_of_cases():
    for mut in AE.MUTANTS:
        n = sum(1 for t in AE.ATTN_CASES if AE.attn_case(*t).applies(mut) is None)
        assert n >= 4, (mut, n)


@pytest.mark.parametrize('half', AE.HALF_MUTANTS)
def test_each_half_of_the_empty_partial_mistake_alone_changes_no_bit(half):
    """P = exp2(s - m) without the validity select, and weight 1 for a partial whose m is still -1e30, are each absorbed by the kernel's design (a partial without a valid key
    merges with weight exp2(-1e30 - max m) = 0; l = 0 and O = 0 take any weight): only the two together ('empty_partial_weight_one') change the output"""
    for t in AE.ATTN_CASES:
        c = AE.attn_case(*t)
        assert torch.equal(c.emul(half)[0], c.emulated[0]), AE.case_id(t)


def test_an_admitted_padding_key_of_zeros_stays_under_the_older_gate_but_a_poisoned_one_does_not():
    """why the pads are poisoned: with zeros in K and V rows [Lk, Lkp), as the older test fills them, a kernel that admits key Lk stays below the older aggregate gate of
    1.2e-2 in every plain case of at least 96 keys; with the poison it is caught outright"""
    for t in AE.ATTN_CASES:
        if t[3] != 'plain' or t[2] < 96:
            continue
        c = AE.attn_case(*t)
        if c.applies('admit_first_pad_key'):
            continue
        z = AE.AttnCase(*t)
        z.k[:, :, c.Lk:] = 0
        z.v[:, :, c.Lk:] = 0
        got = z.emul('admit_first_pad_key')[0][:c.B * c.Lq, :c.D].double()
        ref = c.ref.reshape(c.B * c.Lq, c.D)
        whole = float((got - ref).norm() / ref.norm())
        assert whole < AE.OLD_REL, (t, whole)
        assert AE.caught(_mistake(t, 'admit_first_pad_key'))


def test_the_reference_of_a_case_is_the_plain_softmax_of_each_batch_element_alone():
    c = AE.attn_case('xs', 130, 129, 'kmask', 2)
    for b in range(c.B):
        keys = c.valid[b].nonzero().flatten()
        q, k, v = (x[b, :, :, :c.dh].double() for x in (c.q, c.k, c.v))
        o = torch.softmax(q[:, :c.Lq] @ k[:, keys].transpose(1, 2) / c.dh ** 0.5, -1) @ v[:, keys]
        assert torch.allclose(o.permute(1, 0, 2).reshape(c.Lq, c.D), c.ref[b], rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------------
# refusals of the hooks: everything below returns before the first HIP call and before the handle is looked at (no GPU here)
# ---------------------------------------------------------------------------------------------------
INVALID = -1
_P = 0x1000      # a non-null address that is never followed: each call below is refused first


@pytest.mark.parametrize('varlen', [False, True])
def test_attention_hook_refusals(lib, varlen):
    def call(q=_P, k=_P, v=_P, out=_P, B=2, Lq=130, Lk=130, Lqp=192, Lkp=192, klen=None):
        if varlen:
            return lib.ezdit_test_attention_varlen(None, q, k, v, None, out, B, Lq, Lk, Lqp, Lkp, klen, None)
        return lib.ezdit_test_attention(None, q, k, v, None, out, B, Lq, Lk, Lqp, Lkp, None)
    # a description that is otherwise fine is refused last, for its handle
    assert call() == INVALID and b'null handle' in lib.ezdit_last_error()
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(B=0), dict(B=-1), dict(Lq=0), dict(Lk=0), dict(Lk=-3),
               dict(Lqp=128), dict(Lkp=128), dict(Lqp=129), dict(Lqp=160), dict(Lkp=130), dict(Lkp=224), dict(Lqp=200, Lkp=200)):
        assert call(**kw) == INVALID, kw
        assert b'null handle' not in lib.ezdit_last_error(), kw
    if varlen:
        assert call(Lq=100, klen=_P) == INVALID and b'self-attention' in lib.ezdit_last_error()
