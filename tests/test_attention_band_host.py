"""CPU side of the kernel-level tests of sliding-window self-attention (tests/test_attention_band_gpu.py): the gates of tests/attn_band_emul.py against its fp32 emulation and
its deliberate mistakes, the coverage the cases give the three places that exist only with a band (a masked element under the sentinel max, a key sub-block that ends without a
valid key of a query, a tile loop that does not begin at tile 0), and the refusals of ezdit_test_attention_band that come before the first HIP call."""
import functools

import pytest
import torch

from tests import attn_band_emul as BE
from tests import attn_emul as AE


@functools.lru_cache(maxsize=None)
def _floor(t):
    c = BE.band_case(*t)
    buf, counts = c.emulated
    return c.figures(buf), counts


@pytest.mark.parametrize('case', BE.BAND_CASES, ids=BE.case_id)
def test_emulation_is_clean_and_under_half_of_every_gate(case):
    """per case: the emulation breaks no bitwise check and each gated statistic is at most half its gate.  A gate is AE's unless the case's own floor exceeds half of it; then it
    is recorded in BAND_GATES with that floor, and is twice the floor"""
    f, _ = _floor(case)
    g = BE.gates(case)
    print(BE.case_id(case), f, g)
    assert AE.bitwise_ok(f), f
    for k in ('head', 'row', 'abs'):
        assert f[k] <= g[k] / 2 * 1.005, (k, f[k], g[k])
    own = BE.BAND_GATES.get(BE.case_id(case), {})
    base = dict(head=AE.GATE_HEAD, row=AE.GATE_ROW, abs=AE.GATE_ABS)
    for k in ('head', 'row', 'abs'):
        if k in own:
            gate, floor = own[k]
            assert f[k] > base[k] / 2, (k, 'a gate of its own without need')                  # only where AE's gate is less than twice the floor
            assert 0.98 * floor <= f[k] <= floor * 1.005 and 1.9 * floor <= gate <= 2.005 * floor, (k, f[k], floor, gate)
        else:
            assert g[k] == base[k]


def test_band_gates_name_cases_that_exist():
    ids = {BE.case_id(t) for t in BE.BAND_CASES}
    assert set(BE.BAND_GATES) <= ids


def test_the_cases_reach_what_exists_only_with_a_band():
    """for each NKH: sub-tiles of all three classes, a masked element met under the sentinel max by a real query row, a key sub-block that ends without a valid key of a live query,
    a tile loop that starts behind tile 0 and one that ends before the last tile, and the deferred rescale both firing and deferring beyond the first tile"""
    for nkh in (2, 4):
        for key in ('skipped', 'full', 'mixed', 'sentinel_rows', 'empty_partners', 't_lo_pos', 't_hi_short', 'fired_t1', 'deferred_t1'):
            best = max(_floor(t)[1][key] for t in BE.BAND_CASES if t[4] == nkh)
            print(f'nkh {nkh} {key}: {best} in the best case')
            assert best > 0, (nkh, key)
    # L = 390 at nkh 4 (four key tiles of 128): query tile 4 walks the key tiles [1, 3), neither the first nor the last; query tile 5 begins at key tile 2 (its last queries
    # still reach the keys 384 .. 389 of tile 3)
    c = BE.band_case('xs', 390, 20, None, 4)
    assert max(0, 64 * 4 - 20) // 128 == 1 and (64 * 4 + 63 + 20) // 128 + 1 == 3 and (390 + 127) // 128 == 4
    assert max(0, 64 * 5 - 20) // 128 == 2 and (64 * 5 + 63 + 20) // 128 + 1 == 4
    assert _floor(('xs', 390, 20, None, 4))[1]['t_lo_pos'] > 0 and c.Lkp == 512


@functools.lru_cache(maxsize=None)
def _mistake(t, mut):
    c = BE.band_case(*t)
    return c.figures(c.emul(mut)[0])


def test_every_mistake_is_caught_at_three_times_a_gate_or_by_a_bitwise_check():
    """every mistake of MUTANTS, at EACH key-tile size, in at least one case it can be made in -- and in most of them"""
    for mut in BE.MUTANTS:
        for nkh in (2, 4):
            made = [t for t in BE.BAND_CASES if t[4] == nkh and BE.band_case(*t).applies(mut) is None]
            hit = [t for t in made if BE.caught(_mistake(t, mut), BE.gates(t))]
            print(f'{mut} nkh {nkh}: caught in {len(hit)} of {len(made)} cases; missed in {[BE.case_id(t) for t in made if t not in hit]}')
            assert made and hit, (mut, nkh)
            assert len(hit) >= 0.75 * len(made), (mut, nkh, [BE.case_id(t) for t in made if t not in hit])


@pytest.mark.parametrize('half', BE.HALF_MUTANTS)
def test_each_half_of_the_sentinel_mistake_alone_changes_no_bit(half):
    """weight 1 for a masked element under the sentinel max, and weight 1 in the merge for a partner with lsum = 0, are each absorbed by the kernel's design (BE.HALF_MUTANTS):
    no set of inputs can tell either alone from the kernel, so no case can catch it; the two together are in MUTANTS and are caught"""
    for t in BE.BAND_CASES:
        c = BE.band_case(*t)
        assert torch.equal(c.emul(half)[0], c.emulated[0]), BE.case_id(t)


def test_a_radius_that_covers_the_row_is_the_emulation_of_the_plain_kernel():
    """radius L - 1 masks nothing: every entered sub-tile below L is FULL or ends at L, and the reference is the plain softmax"""
    for t in BE.BAND_CASES:
        if t[2] < t[1] - 1:
            continue
        c = BE.band_case(*t)
        assert _floor(t)[1]['skipped'] == 0
        q, k, v = (x[:, :, :c.Lq, :c.dh].double() for x in (c.q, c.k, c.v))
        o = (torch.softmax(q @ k.transpose(2, 3) / c.dh ** 0.5, -1) @ v).permute(0, 2, 1, 3).reshape(c.B, c.Lq, c.D)
        assert torch.allclose(o, c.ref, rtol=0, atol=1e-12)


def test_the_reference_is_the_softmax_over_each_row_s_own_keys():
    c = BE.band_case('xs', 260, 20, BE.KLEN6, 2)
    for b, n in enumerate(c.lk_b):
        for i in (0, 19, 20, 21, 179, 180, 199):
            keys = [j for j in range(c.Lq) if abs(i - j) <= 20 and j < n]
            q, k, v = (x[b, :, :, :c.dh].double() for x in (c.q, c.k, c.v))
            o = torch.softmax(q[:, i:i + 1] @ k[:, keys].transpose(1, 2) / c.dh ** 0.5, -1) @ v[:, keys]
            assert torch.allclose(o.reshape(c.D), c.ref[b, i], rtol=0, atol=1e-12), (b, i)
        assert bool((c.ref[b, n:] == 0).all())


# ---------------------------------------------------------------------------------------------------
# refusals of the hook: everything below returns before the first HIP call and before the handle is looked at (no GPU here)
# ---------------------------------------------------------------------------------------------------
INVALID = -1
_P = 0x1000      # a non-null address that is never followed: each call below is refused first


def test_band_hook_refusals(lib):
    def call(q=_P, k=_P, v=_P, out=_P, B=2, L=130, Lp=192, klen=None, radius=20):
        return lib.ezdit_test_attention_band(None, q, k, v, out, B, L, Lp, klen, radius, None)
    assert call() == INVALID and b'null handle' in lib.ezdit_last_error()      # a description that is otherwise fine is refused last, for its handle
    for kw in (dict(radius=0), dict(radius=-1), dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(B=0), dict(L=0), dict(Lp=128), dict(Lp=130), dict(Lp=160),
               dict(Lp=200)):
        assert call(**kw) == INVALID, kw
        assert b'null handle' not in lib.ezdit_last_error(), kw
    assert call(radius=0) == INVALID and b'radius' in lib.ezdit_last_error()
