"""CPU side of the kernel-level tests of the streaming kernels (tests/test_row_kernels_gpu.py): the gates of tests/row_emul.py against its fp32 emulation and its
deliberate mistakes, and the refusals of the three hooks (ezdit_test_row, ezdit_test_headnorm, ezdit_test_assemble), which all come before the first HIP call."""
import ctypes as C

import pytest
import torch

from tests import row_emul as RE


def _row_figures(c, h, u):
    """(worst |h - ref| / bound, worst row rel-L2 of u, worst excess of u over half an ulp in units of |ln_g| + |ln_c|)"""
    h64, u64 = c.ref
    bound = c.h_bound()
    hr = float(((h.double() - h64).abs() / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else float((h.double() - h64).abs().max())
    return hr, RE.worst_row_rel(u, u64), RE.u_excess(u, u64, c.u_scale())


@pytest.mark.parametrize('spec', RE.ROW_CASES, ids=RE.row_id)
def test_row_gates_hold_the_emulation_and_catch_every_mistake(spec):
    """The fp32 emulation (reciprocal square root exact, one ulp low, one ulp high) stays within half of the h_out bound and of A_REL and at its floor under the capped
    rel-L2 gate (twice the floor is above the cap, as for the capped gates of tests/kernel_emul.py); every mistake of ROW_MUTANTS that can be made in the case lands at three
    times the gate meant for it: the h_out bound for the mistakes the fp32 stream shows (where h_out is stored), else BOTH the worst-row rel-L2 and the elementwise bound of
    u.  A mistake that cannot be made is skipped by name (RowCase.applies gives the reason)."""
    c = RE.row_case(spec)
    gate, floor = (RE.GATE_ROW_U_D4, RE.FLOOR_ROW_U_D4) if c.D == 4 else (RE.GATE_ROW_U, RE.FLOOR_ROW_U)
    for h, u in c.emul3:
        hr, wr, ex = _row_figures(c, h, u)
        assert not torch.isnan(u).any() and not torch.isnan(h).any()
        assert hr <= 0.5 and ex <= RE.A_REL / 2 and wr <= floor * 1.005 < gate, (hr, wr, ex)
    if 'constant' in c.rows and c.exact_rows:
        r = c.rows['constant']
        assert torch.equal(c.emul()[1][r], RE.bf16r(c.ln_c[c.slot[r], :c.width]))
    skipped = {}
    for mut in RE.ROW_MUTANTS:
        why = c.applies(mut)
        if why:
            skipped[mut] = why
            continue
        hr, wr, ex = _row_figures(c, *c.emul(mut))
        if mut in RE.H_MUTANTS and c.h_out:
            assert hr >= 3, (mut, hr)
        else:
            assert wr >= 3 * gate and ex >= 3 * RE.A_REL, (mut, wr, ex)
    print('skipped:', skipped)


def test_no_more_than_a_quarter_of_the_row_case_mistake_pairs_is_skipped():
    pairs = [(RE.row_id(s), m, RE.row_case(s).applies(m)) for s in RE.ROW_CASES for m in RE.ROW_MUTANTS]
    skipped = [p for p in pairs if p[2]]
    print(f'{len(skipped)} of {len(pairs)} (case, mistake) pairs skipped')
    assert len(skipped) <= len(pairs) / 4
    for m in RE.ROW_MUTANTS:      # and every mistake is made in a fair number of cases
        assert sum(1 for p in pairs if p[1] == m and not p[2]) >= 20, m


@pytest.mark.parametrize('spec', [s for s in RE.ROW_CASES if s['M'] >= 1024 and s['D'] == 1152], ids=RE.row_id)
def test_a_lost_chunk_of_the_variance_shows_per_row_but_not_over_the_whole_matrix(spec):
    """why u is gated per row: a variance without its last four columns is wrong by a quarter in the one row built to show it (the spike row) -- fifty times the gate -- and
    stays under three times the gate in the rel-L2 over the thousand rows of the matrix, where a mistake has to land to count as caught"""
    c = RE.row_case(spec)
    u = c.emul('last_chunk_out_of_variance')[1]
    whole, worst = RE.rel_l2(u, c.ref[1]), RE.worst_row_rel(u, c.ref[1])
    assert whole < 3 * RE.GATE_ROW_U and worst >= 40 * RE.GATE_ROW_U, (whole, worst)


@pytest.mark.parametrize('case', RE.HEAD_CASES, ids=lambda t: 'H%d-dh%d-B%d-L%d-Lp%d-%s' % t)
def test_headnorm_gate_holds_the_emulation_and_catches_every_mistake(case):
    c = RE.head_case(*case)
    qk = [n for n in c.parts() if n != 'v']
    for em in c.emul3:
        assert max(RE.per_head_rel_qk(em[n], c.ref[n]) for n in qk) <= RE.FLOOR_HEAD * 1.005 < RE.GATE_HEAD
        if 'v' in em:
            assert torch.equal(em['v'], RE.bf16r(c.ref['v'].float()))
    skipped = {}
    for mut in RE.HEAD_MUTANTS:
        why = c.applies(mut)
        if why:
            skipped[mut] = why
            continue
        bad = c.emul(mut)
        w = max(RE.per_head_rel_qk(bad[n], c.ref[n]) for n in qk)
        assert w >= 3 * RE.GATE_HEAD, (mut, w)
    print('skipped:', skipped)


def test_every_headnorm_mistake_is_made_in_a_fair_number_of_cases():
    """(rope_on_when_null excludes the two RoPE mistakes and ln_over_dqk exists at head_dim 72 only: no case can hold more than five of the six)"""
    for m in RE.HEAD_MUTANTS:
        assert sum(1 for hc in RE.HEAD_CASES if not RE.head_case(*hc).applies(m)) >= 8, m


def test_assembly_cases_expect_nothing_non_finite():
    for ac in RE.ASM_CASES:
        c = RE.AsmCase(*ac)
        e = c.expected()
        assert torch.isfinite(e).all() and e.shape == (c.B * c.L, c.ldo)
        assert torch.isnan(c.x).any() == (c.L > 1 and (c.form == 'pre' or c.x_rows > 1))      # (the NaN beyond the lengths are there to be kept out)


# ---------------------------------------------------------------------------------------------------
# refusals of the hooks: everything below returns before the first HIP call (no GPU here)
# ---------------------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -2
_P = 0x1000      # a non-null, 16-byte aligned address that is never followed: each call below is refused first


def _row_args(**kw):
    from ezaudio_amd import _lib
    a = _lib.EzditTestRowArgs()
    base = dict(h_in=_P, h_out=_P, part=_P, nsplit=2, ld_part=64, part_stride=64 * 16, part_bf16=1, mode=1, bias=_P, gate=_P, gate_slot_stride=64,
                ln_g=_P, ln_c=_P, ln_slot_stride=64, u=_P, ld_u=64, M=8, D=64, L=8, n_slots=0)      # n_slots = 0: a description that is otherwise fine is refused last
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_row_hook_refusals(lib):
    row = lambda **kw: lib.ezdit_test_row(C.byref(_row_args(**kw)), None)
    assert lib.ezdit_test_row(None, None) == INVALID
    assert row() == INVALID and b'n_slots' in lib.ezdit_last_error()      # the base description passes every check up to the slots
    for kw in (dict(D=66), dict(D=2052, ld_part=2052, ld_u=2052), dict(nsplit=9)):
        assert row(**kw) == UNSUPPORTED, kw
    for kw in (dict(nsplit=-1), dict(M=0), dict(D=0), dict(L=0), dict(mode=3),
               dict(h_in=None), dict(part=None), dict(mode=2, part=None), dict(ln_g=None), dict(ln_c=None),       # a pointer the mode needs
               dict(ld_u=60), dict(ld_u=66), dict(skip=_P, ld_u=64),                                               # below the written width, not a multiple of 4
               dict(ld_part=60), dict(ld_part=66), dict(part_stride=1026), dict(gate_slot_stride=66), dict(ln_slot_stride=66), dict(part_stride=0),
               dict(cn=_P), dict(skip=_P, ld_u=128, u=None), dict(h_in=_P + 4), dict(u=_P + 4), dict(part=_P + 4), dict(variant=2)):
        assert row(**kw) == INVALID, kw
        assert b'n_slots' not in lib.ezdit_last_error(), kw
    # what the other modes do NOT need is not asked for
    for kw in (dict(mode=2, h_in=None), dict(mode=0, part=None, gate=None, bias=None), dict(nsplit=0, part=None), dict(u=None, ln_g=None, ln_c=None)):
        assert row(**kw) == INVALID and b'n_slots' in lib.ezdit_last_error(), kw


def test_headnorm_hook_refusals(lib):
    def hn(ldx=3 * 128, q_col=0, k_col=128, v_col=256, x=_P, qa=_P, ka=_P, rope=(None, None), q=_P, k=_P, v=_P, B=1, H=2, L=4, Lp=64, dh=64):
        return lib.ezdit_test_headnorm(x, ldx, q_col, k_col, v_col, qa, qa, ka, ka, rope[0], rope[1], q, k, v, B, H, L, Lp, dh, None)
    for kw in (dict(dh=80), dict(dh=32), dict(dh=0)):
        assert hn(**kw) == UNSUPPORTED, kw
    for kw in (dict(Lp=3), dict(ldx=385), dict(ldx=386), dict(q_col=1), dict(k_col=129), dict(v_col=258), dict(ldx=300), dict(x=None), dict(q=None), dict(qa=None),
               dict(k=None), dict(ka=None), dict(v=None), dict(q_col=-1, k_col=-1, v_col=-1), dict(rope=(_P, None)), dict(B=0), dict(v=_P + 8)):
        assert hn(**kw) == INVALID, kw
    assert hn(ldx=258, v_col=-1, q_col=0, k_col=132) == INVALID      # k does not fit


def test_assemble_hook_refusals(lib):
    def asm(x=_P, x_rows=2, in_ch=8, gt=None, gm=None, me=_P, out=_P, ldo=64, B=4, C=8, L=5):
        return lib.ezdit_test_assemble(x, x_rows, in_ch, gt, gm, me, out, ldo, B, C, L, None, None)
    for kw in (dict(in_ch=9), dict(in_ch=16), dict(x_rows=3), dict(x_rows=0), dict(gt=_P), dict(gm=_P), dict(ldo=16), dict(in_ch=17, ldo=16), dict(x=None), dict(out=None),
               dict(me=None), dict(B=0), dict(L=0)):
        assert asm(**kw) == INVALID, kw
