"""CPU side of the kernel-level tests of the once-per-call tables (tests/test_call_tables_gpu.py): the gates of tests/table_emul.py against its fp32 emulations and its
deliberate mistakes.  The reference alone (the emulation without a mistake) stays inside every hard bound and at its recorded floor; every listed mistake lies at least
MUT_FACTOR = 10 gates (10 x the hard bound in its worst element) from the reference on the fixtures the GPU tests run."""
import numpy as np
import pytest

from tests import table_emul as TE

SLOTS_33 = tuple(range(999, 999 - 33 * 30, -30))      # 33 slots: 132 operand rows, the smallest count that crosses the 128-row tile of the table GEMM
f32, f64 = np.float32, np.float64


@pytest.mark.parametrize('name', TE.FIXTURES)
def test_chain_floors_are_the_recorded_ones_and_every_mistake_lies_ten_gates_off(name):
    fx = TE.fixture(name)
    ref, fl = TE.floors(fx, TE.SLOTS_A)
    for t in TE.chain_tables(fx):
        rec = np.array(TE.FLOORS_A[name][t])
        print(name, t, ' '.join('%.3e' % v for v in fl[t]))
        assert np.all(fl[t] <= 1.5 * rec) and np.all(fl[t] >= rec / 1.5), (t, fl[t], rec)
        # orientation of the issue: about 1.5e-7 at t <= 1, up to 4.2e-5 at t = 999
        assert fl[t].max() < 6e-5 and fl[t][-2:].max() < 3e-7
    for mut in TE.TIME_MUTANTS + TE.MOD_MUTANTS:
        why = TE.applies_chain(fx, len(TE.SLOTS_A), mut)
        if why:
            print('skipped:', mut, why)
            continue
        d = TE.chain_distances(fx, TE.emul_chain(fx, TE.SLOTS_A, 0, mut), ref)
        worst = max(float((d[t] / (TE.CHAIN_FACTOR * fl[t])).max()) for t in d)
        assert worst >= TE.MUT_FACTOR, (mut, worst)


def test_every_chain_mistake_is_made_on_some_fixture():
    for mut in TE.TIME_MUTANTS + TE.MOD_MUTANTS:
        assert any(TE.applies_chain(TE.fixture(n), len(TE.SLOTS_A), mut) is None for n in TE.FIXTURES), mut
    # the scaling can be told only where it is not 1: that is what the alpha = 6 fixture is for
    assert [n for n in TE.FIXTURES if TE.applies_chain(TE.fixture(n), 6, 'lora_unscaled') is None] == ['xs_a6']
    assert TE.fixture('xs_a6').scaling == 1.5


@pytest.mark.parametrize('n', (1, 4, 5, 33))
def test_chain_mistakes_of_the_slot_path_show_at_every_slot_count(n):
    """the two mistakes that depend on the slot count: a lost chunk tail needs a partial chunk behind a full one (n = 5), the neighbour's slot more than one slot"""
    fx = TE.fixture('xs')
    ts = SLOTS_33[:n]
    ref, fl = TE.floors(fx, ts)
    for mut in ('neighbour_slot', 'chunk_tail_lost'):
        if TE.applies_chain(fx, n, mut):
            continue
        d = TE.chain_distances(fx, TE.emul_chain(fx, ts, 0, mut), ref)
        assert max(float((d[t] / (TE.CHAIN_FACTOR * fl[t])).max()) for t in d) >= TE.MUT_FACTOR, mut
    assert TE.applies_chain(fx, 5, 'chunk_tail_lost') is None and TE.applies_chain(fx, 6, 'chunk_tail_lost') is None


@pytest.mark.parametrize('name', TE.FIXTURES)
def test_linear_bound_holds_the_emulation(name):
    """every k_linear_f32 launch of the chain, isolated: the emulated output against the fp64 product of the emulation's OWN input"""
    fx = TE.fixture(name)
    m = fx.prefix
    em = TE.emul_chain(fx, TE.SLOTS_A)
    launches = [('tt', em['t1'], fx.p(m + 'time_embed.mlp.2.weight'), fx.p(m + 'time_embed.mlp.2.bias'), True, em['tt']),
                ('ada', em['tt'], fx.p(m + 'time_ada.weight'), fx.p(m + 'time_ada.bias'), False, em['ada'])]
    if fx.has_final:
        launches.append(('adaf', em['tt'], fx.p(m + 'time_ada_final.weight'), fx.p(m + 'time_ada_final.bias'), False, em['adaf']))
    for b in range(fx.nblk):
        la = TE.lin_emul(em['tt'], fx.blk(b, 'adaln.lora_a.weight'))
        launches.append((f'la{b}', em['tt'], fx.blk(b, 'adaln.lora_a.weight'), None, False, la))
        launches.append((f'lora{b}', la, fx.blk(b, 'adaln.lora_b.weight'), None, False, em['lora'][:, b]))
    for what, x, W, bias, act, got in launches:
        ref = TE.lin_ref(x, W, bias, act)
        r = TE.worst_ratio(got, ref, TE.lin_bound(x, W, bias, act, ref))
        print(name, what, '%.3f' % r)
        assert r <= 0.5, (what, r)
        # ... and the bound is a bound on THIS launch: the slot before (a neighbour's row) is ten bounds off
        if len(got) > 1:
            assert TE.worst_ratio(np.roll(got, 1, 0), ref, TE.lin_bound(x, W, bias, act, ref)) >= TE.MUT_FACTOR, what


@pytest.mark.parametrize('name', TE.FIXTURES)
def test_fold_bound_holds_the_emulation_and_catches_every_mistake(name):
    fx = TE.fixture(name)
    em = TE.emul_chain(fx, TE.SLOTS_A)
    mb, fb = TE.fold_bound(fx, em['ada'], em['lora'], em.get('adaf'))
    ref = TE.fold(fx, TE.six_of(fx, em['ada'].astype(f64), em['lora'].astype(f64), f64), f64)
    r = TE.worst_ratio(em['mod'], ref, mb)
    print(name, 'mod %.3f' % r)
    assert r <= 1.0
    reff = None
    if fx.has_final:
        reff = TE.fold_final(fx, em['adaf'].astype(f64), f64)
        assert TE.worst_ratio(em['modf'], reff, fb) <= 1.0
    for mut in TE.MOD_MUTANTS:
        if TE.applies_chain(fx, len(TE.SLOTS_A), mut):
            continue
        if mut == 'final_shift_scale_swapped':
            r = TE.worst_ratio(TE.fold_final(fx, em['adaf'], f32, mut), reff, fb)
        else:
            r = TE.worst_ratio(TE.fold(fx, TE.six_of(fx, em['ada'], em['lora'], f32, mut), f32, mut), ref, mb)
        assert r >= TE.MUT_FACTOR, (mut, r)


@pytest.mark.parametrize('n', (6, 33))
@pytest.mark.parametrize('name', TE.FIXTURES)
def test_table_bound_holds_the_emulation_and_catches_every_mistake(name, n):
    """G' / C': the emulation stays an order of magnitude inside the bound, every mistake lands ten bounds outside in each table it touches"""
    fx = TE.fixture(name)
    mod = TE.emul_chain(fx, TE.SLOTS_A if n == 6 else SLOTS_33)['mod']
    r = TE.zt_ratios(fx, mod, TE.zt_emul(fx, mod))
    print(name, n, {k: '%.3f' % v for k, v in r.items()})
    assert max(r.values()) <= 0.2, r
    for mut in TE.ZT_MUTANTS:
        why = TE.applies_zt(fx, n, mut)
        if why:
            print('skipped:', mut, why)
            continue
        r = TE.zt_ratios(fx, mod, TE.zt_emul(fx, mod, mut))
        for which in TE.ZT_MUTANT_TABLES[mut]:
            if which in r:
                assert r[which] >= TE.MUT_FACTOR, (mut, which, r[which])


def test_every_table_mistake_is_made_on_some_fixture():
    for mut in TE.ZT_MUTANTS:
        assert any(TE.applies_zt(TE.fixture(nm), n, mut) is None for nm in TE.FIXTURES for n in (6, 33)), mut
    assert TE.applies_zt(TE.fixture('xs'), 32, 'rows_past_128_lost') and not TE.applies_zt(TE.fixture('xs'), 33, 'rows_past_128_lost')


@pytest.mark.parametrize('B', (4, 34))
@pytest.mark.parametrize('name', TE.FIXTURES)
def test_zd_bound_holds_the_emulation_and_catches_every_mistake(name, B):
    fx = TE.fixture(name)
    Lc = 20
    mask, key1 = TE.zd_masks(B, Lc)
    el = np.nonzero(key1 >= 0)[0]
    assert key1[B - 1] > 0 and len(el) == (2 if B == 4 else 33) and (B == 4 or len(el) > TE.GEMV_MAXB)
    if B == 4:
        assert mask.sum(1).tolist() == [1, 6, 20, 1]
    _, ckv = TE.zd_ckv(name, B, Lc)
    v = TE.bf16r(np.stack([ckv[b, el, key1[el], fx.D:] for b in range(fx.nblk)]))
    ref, bound = TE.zd_ref_bound(fx, v)
    r = TE.worst_ratio(TE.zd_emul(fx, ckv, key1), ref, bound)
    print(name, B, '%.4f' % r)
    assert r <= 0.5
    for mut in TE.ZD_MUTANTS:
        if TE.applies_zd(fx, mut):
            continue
        r = TE.worst_ratio(TE.zd_emul(fx, ckv, key1, mut), ref, bound)
        assert r >= TE.MUT_FACTOR, (mut, r)


def test_bf16_rounding_and_ulp_bound():
    import torch
    x = np.concatenate([np.random.default_rng(3).standard_normal(4096).astype(f32) * 3, np.array([0, 1, -1, 1.00390625, 1.01171875, 1.9999999], f32)])
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(TE.bf16r(x), want)
    assert np.all(np.abs(want.astype(f64) - x) <= TE.bf16_ulp_bound(x.astype(f64)) / 2)
    # two ulps off is outside
    two = (want.view(np.uint32) + np.uint32(2 << 16)).view(f32)
    nz = x != 0
    assert np.all(np.abs(two.astype(f64) - x)[nz] > TE.bf16_ulp_bound(x.astype(f64))[nz])


def _emulated_workspace(fx, ts, mut=None, em=None):
    """the buffers tests/test_call_tables_gpu.py reads back, from the emulation (with one mistake); `em`: the chain without a mistake, where it is at hand"""
    if em is None or mut in TE.TIME_MUTANTS + TE.MOD_MUTANTS:
        em = TE.emul_chain(fx, ts, 0, mut if mut in TE.TIME_MUTANTS + TE.MOD_MUTANTS else None)
    zt = TE.zt_emul(fx, em['mod'], mut if mut in TE.ZT_MUTANTS else None)
    n, D = len(ts), fx.D
    buf = dict(em, la=TE.lin_emul(em['tt'], fx.blk(fx.nblk - 1, 'adaln.lora_a.weight')), zt_qkv=zt['qkv'], zt_geglu=zt['geglu'], zt_q2=zt['q2'],
               zt_skip=zt.get('skip', np.zeros((1, 2, D), f32)))
    if not fx.has_final:
        buf.update(adaf=np.zeros((n, 2 * D), f32), modf=np.zeros((n, 2, D), f32))
    return buf


@pytest.mark.parametrize('name', ('xs_a6', 'cn_xs'))
def test_the_gpu_tests_check_passes_the_emulation_and_refuses_every_mistake(name, monkeypatch):
    """the checking code of the GPU tests itself, fed from the emulation instead of the device: it passes the emulated workspace and raises on each mistake (the mistakes of
    the chain at six slots, those of the tables at 33)"""
    import tests.test_call_tables_gpu as G
    monkeypatch.setattr(G, 'record', lambda line: None)
    fx = TE.fixture(name)
    made = 0
    for ts, muts in ((TE.SLOTS_A, TE.TIME_MUTANTS + TE.MOD_MUTANTS), (SLOTS_33, TE.ZT_MUTANTS)):
        em = TE.emul_chain(fx, ts)
        G.check(fx, ts, _emulated_workspace(fx, ts, None, em), 'emulation')
        for mut in muts:
            if TE.applies_chain(fx, len(ts), mut) or TE.applies_zt(fx, len(ts), mut):
                continue
            with pytest.raises(AssertionError):
                G.check(fx, ts, _emulated_workspace(fx, ts, mut, em), mut)
            made += 1
    assert made >= (19 if name == 'xs_a6' else 14)
