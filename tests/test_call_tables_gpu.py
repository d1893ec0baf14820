"""Kernel-level GPU tests of the once-per-call tables: what ezdit_prepare_timesteps (time path, AdaLN-SOLA modulation folded with the LayerNorm affine, the LayerNorm-algebra
tables G' / C') and ezdit_prepare_context (the single-key vector zd, the bf16 casts of the context path) leave in the workspace, read through debug_buffer and judged against
the fp64 references of tests/table_emul.py.  The kernels: k_linear_f32, k_mod_finalize, k_z_hilo, k_z_combine, k_gemv_bf16w, k_cast_bf16 (csrc/rowops.hip).

Two kinds of check (tests/table_emul.py has the gates and the numbers behind them, tests/test_call_tables_host.py their CPU side):
  chain      tt, ada, adaf, mod, modf against the fp64 oracle from the timesteps: rel-L2 per (timestep, table) <= 2 x the emulated floor of that timestep
  isolated   one kernel under test, its inputs read back from the device: elementwise bounds with nothing measured

The models are private to this module (the tests poison workspaces), xs (D 144) and xs64 (D 128) at depth 2, one xs with ada_sola_alpha = 6 (scaling 1.5), one ControlNet
handle.  No option is set.  Every measured distance goes to the parity log (tests.util.record)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import table_emul as TE
from tests.util import record

pytestmark = pytest.mark.gpu

L, LC = 16, 20
SLOTS_33 = tuple(range(999, 999 - 33 * 30, -30))
SLOT_TABLES = ('t1', 'tt', 'ada', 'adaf', 'la', 'lora', 'mod', 'modf', 'zt_qkv', 'zt_geglu')      # slot-indexed: [n_slots][...]
POISONED = SLOT_TABLES + ('zA', 'ztmp', 'zt_q2', 'zt_skip')      # what ezdit_prepare_timesteps alone writes (ezdit_bind_workspace zeroes the whole workspace and fills
                                                                  # the RoPE tables: it initialises none of these to anything but that zero)
f32, f64 = np.float32, np.float64
_models = {}


def model(name):
    from ezaudio_amd import DiTControlNet, MaskDiT
    from oracle.controlnet import CN_DEFAULT
    if name not in _models:
        fx = TE.fixture(name)
        if fx.is_cn:
            cfg = dict(fx.cfg)
            cfg.update(CN_DEFAULT)
            m = DiTControlNet(device='cuda:0', **cfg)
        else:
            m = MaskDiT(device='cuda:0', **fx.cfg)
        m.load_state_dict(fx.sd)
        _models[name] = m
    return _models[name]


def rebind(m, B, n_slots, Lx=L):
    m._ws_key = None      # a fresh binding every time: the workspace is zeroed again
    m.bind(B, Lx, LC, n_slots)


def region(m, name):
    """the bytes of workspace buffer `name`, in place, through the offset ezdit_debug_buffer reports"""
    p, n = C.c_void_p(), C.c_size_t()
    assert m.lib.ezdit_debug_buffer(m._h, name.encode(), C.byref(p), C.byref(n)) == 0
    off = p.value - m._ws.data_ptr()
    return m._ws[off:off + n.value]


def read(m, fx, ns):
    D, nb, I = fx.D, fx.nblk, fx.I
    torch.cuda.synchronize()
    shapes = dict(t1=(ns, D), tt=(ns, D), ada=(ns, 6 * D), adaf=(ns, 2 * D), la=(ns, fx.r6), lora=(ns, nb, 6 * D), mod=(ns, nb, 6, D), modf=(ns, 2, D),
                  zt_qkv=(ns, nb, 2, 3 * D), zt_geglu=(ns, nb, 2, 2 * I), zt_q2=(nb, 2, D), zt_skip=(max(fx.nhalf, 1), 2, D))
    return {k: m.debug_buffer(k, torch.float32, s).cpu().numpy() for k, s in shapes.items()}


def check(fx, ts, buf, what):
    """chain and isolated checks of the first len(ts) slots of every table"""
    n = len(ts)
    ref, fl = TE.floors(fx, ts)
    for t in TE.chain_tables(fx):
        assert np.isfinite(buf[t][:n]).all(), (what, t)
        d = TE.rel_rows(buf[t][:n], ref[t])
        k = int(np.argmax(d / fl[t]))
        record(f'{what} chain {t}: worst rel-L2 / floor {d[k] / fl[t][k]:.2f} at t = {ts[k]} ({d[k]:.3e} against floor {fl[t][k]:.3e}); largest rel-L2 {d.max():.3e}')
        assert np.all(d <= TE.CHAIN_FACTOR * fl[t]), (what, t, d, fl[t])
    m = fx.prefix
    lin = [('tt', buf['t1'], fx.p(m + 'time_embed.mlp.2.weight'), fx.p(m + 'time_embed.mlp.2.bias'), True, buf['tt']),
           ('ada', buf['tt'], fx.p(m + 'time_ada.weight'), fx.p(m + 'time_ada.bias'), False, buf['ada']),
           ('la', buf['tt'], fx.blk(fx.nblk - 1, 'adaln.lora_a.weight'), None, False, buf['la']),          # (`la` holds the last block's)
           ('lora', buf['la'], fx.blk(fx.nblk - 1, 'adaln.lora_b.weight'), None, False, buf['lora'][:, fx.nblk - 1])]
    if fx.has_final:
        lin.append(('adaf', buf['tt'], fx.p(m + 'time_ada_final.weight'), fx.p(m + 'time_ada_final.bias'), False, buf['adaf']))
    ratios = {}
    for nm, x, W, b, act, got in lin:
        r64 = TE.lin_ref(x[:n], W, b, act)
        ratios[nm] = TE.worst_ratio(got[:n], r64, TE.lin_bound(x[:n], W, b, act, r64))
    ada, lora = buf['ada'][:n], buf['lora'][:n]
    mb, fb = TE.fold_bound(fx, ada, lora, buf['adaf'][:n] if fx.has_final else None)
    ratios['mod'] = TE.worst_ratio(buf['mod'][:n], TE.fold(fx, TE.six_of(fx, ada.astype(f64), lora.astype(f64), f64), f64), mb)
    if fx.has_final:
        ratios['modf'] = TE.worst_ratio(buf['modf'][:n], TE.fold_final(fx, buf['adaf'][:n].astype(f64), f64), fb)
    zt = dict(qkv=buf['zt_qkv'][:n], geglu=buf['zt_geglu'][:n], q2=buf['zt_q2'], skip=buf['zt_skip'])
    ratios.update({'zt_' + k: v for k, v in TE.zt_ratios(fx, buf['mod'][:n], zt).items()})
    record(f'{what} isolated, worst |got - ref64| / bound: ' + ' '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (what, k, v)


def prepare(m, ts, per_row=False):
    m.prepare_timesteps([int(t) for t in ts], per_row)


# ---- (a) chain and isolated checks at the six slots, both widths and scaling 1.5 ----
@pytest.mark.parametrize('name', ('xs', 'xs64', 'xs_a6'))
def test_tables_of_six_slots(name):
    fx, m = TE.fixture(name), model(name)
    rebind(m, 2, len(TE.SLOTS_A))
    prepare(m, TE.SLOTS_A)
    check(fx, TE.SLOTS_A, read(m, fx, len(TE.SLOTS_A)), f'(a) {name} n=6')


# ---- (b) slot counts: one, a full chunk, a chunk and one, 132 operand rows (the 128-row tile of the table GEMM crossed) ----
@pytest.mark.parametrize('n', (1, 4, 5, 33))
@pytest.mark.parametrize('name', ('xs', 'xs64'))
def test_every_slot_of_every_table(name, n):
    fx, m = TE.fixture(name), model(name)
    rebind(m, 2, n)
    prepare(m, SLOTS_33[:n])
    check(fx, SLOTS_33[:n], read(m, fx, n), f'(b) {name} n={n}')


# ---- (c) slot independence of the fp32 kernels, bit for bit ----
def test_a_slot_is_what_its_timestep_gives_alone():
    fx, m = TE.fixture('xs'), model('xs')
    n = len(TE.SLOTS_A)
    names = ('tt', 'ada', 'adaf', 'lora', 'mod', 'modf')
    rebind(m, n, n)
    prepare(m, TE.SLOTS_A)
    full = read(m, fx, n)
    for s, t in enumerate(TE.SLOTS_A):
        prepare(m, [t])
        one = read(m, fx, n)
        for k in names:
            assert np.array_equal(full[k][s].view(np.uint32), one[k][0].view(np.uint32)), (k, s, t)
        check(fx, [t], one, f'(c) xs t={t} alone')
    prepare(m, TE.SLOTS_A, per_row=True)      # per_row = 1 (n == B) fills the same tables from the same list
    rows = read(m, fx, n)
    for k in names:
        assert np.array_equal(full[k].view(np.uint32), rows[k].view(np.uint32)), k
    check(fx, TE.SLOTS_A, rows, '(c) xs per_row')


# ---- (d) poison: nothing of the call's slots is left unwritten, nothing behind them is touched ----
def test_poisoned_workspace():
    fx, m = TE.fixture('xs'), model('xs')
    n, ns = len(TE.SLOTS_A), 8
    rebind(m, 2, ns)
    for k in POISONED:
        assert not region(m, k).any(), k      # the binding left nothing here but its zero fill
        region(m, k).fill_(0xFF)
    prepare(m, TE.SLOTS_A)
    first = read(m, fx, ns)
    check(fx, TE.SLOTS_A, first, '(d) xs n=6 of 8 poisoned slots')
    for k in SLOT_TABLES:
        assert np.isfinite(first[k][:n]).all(), k
        assert np.all(first[k][n:].view(np.uint32) == 0xFFFFFFFF), k
    ts2 = (7, 500, 250)
    prepare(m, ts2)
    second = read(m, fx, ns)
    check(fx, ts2, second, '(d) xs n=3 behind n=6')
    for k in SLOT_TABLES:
        assert np.array_equal(second[k][3:].view(np.uint32), first[k][3:].view(np.uint32)), k


# ---- (e), (f) the static tables and the GEGLU table ----
@pytest.mark.parametrize('name', ('xs', 'xs64'))
def test_static_and_geglu_tables(name):
    fx, m = TE.fixture(name), model(name)
    ts = (499, 19)
    rebind(m, 2, len(ts))
    prepare(m, ts)
    buf = read(m, fx, len(ts))
    mod = buf['mod']
    far = {}
    for which, item, b in TE.zt_items(fx):
        if which == 'qkv':
            continue
        ref, bound = TE.zt_ref_bound(fx, mod, which, b)
        got = buf['zt_geglu'][:, item] if which == 'geglu' else buf['zt_' + which][item][None]
        r = TE.worst_ratio(got, ref, bound)
        record(f'(e,f) {name} {which} item {item}: worst |got - ref64| / bound {r:.3f}')
        assert r <= 1.0, (which, item, r)
        W, bias = TE.packed(fx, b, which)
        if which == 'q2':
            assert bias is None      # norm2 -> to_q has no bias: C' is c W^T alone, which the reference above states
        else:       # C' carries the bias (b1 in the packed order, skip_linear.bias): without it the table is far outside
            nobias = ref.copy()
            nobias[:, 1] -= bias.astype(f64)
            far[which + ' without bias'] = min(far.get(which + ' without bias', np.inf), TE.worst_ratio(got, nobias, bound))
        if which == 'geglu':      # columns in the packed 8 + 8 order: the natural order is far outside
            Wn, bn = TE.packed(fx, b, which, natural=True)
            g, c = TE.zt_sources(fx, mod, b, which)
            nat = np.stack([g.astype(f64) @ Wn.astype(f64).T, c.astype(f64) @ Wn.astype(f64).T + bn.astype(f64)], 1)
            far['geglu in natural order'] = min(far.get('geglu in natural order', np.inf), TE.worst_ratio(got, nat, bound))
    record(f'(e,f) {name} distance to the mistaken references in bounds: ' + ' '.join(f'{k}: {v:.0f}' for k, v in far.items()))
    assert all(v >= TE.MUT_FACTOR for v in far.values()), far
    if not fx.is_cn:
        assert 'skip without bias' in far


# ---- (g) the ControlNet handle: no final block ----
def test_controlnet_handle():
    fx, m = TE.fixture('cn_xs'), model('cn_xs')
    n = len(TE.SLOTS_A)
    rebind(m, 2, n)
    prepare(m, TE.SLOTS_A)
    buf = read(m, fx, n)
    check(fx, TE.SLOTS_A, buf, '(g) cn_xs n=6')
    for k in ('adaf', 'modf', 'zt_skip'):      # never written on this handle: as the binding left them
        assert not buf[k].any(), k


# ---- (h) zd and the casts of the context path ----
@pytest.mark.parametrize('B', (4, 34))
@pytest.mark.parametrize('name', ('xs', 'xs64'))
def test_single_key_vector_and_context_casts(name, B):
    fx, m = TE.fixture(name), model(name)
    D, H, dh, nb = fx.D, fx.cfg['num_heads'], fx.dh, fx.nblk
    DV, Lcp, ldD = (64 if dh == 64 else 96), 128, (D + 63) // 64 * 64
    mask, key1 = TE.zd_masks(B, LC)
    ctx, _ = TE.zd_ckv(name, B, LC)
    rebind(m, B, 1, Lx=8)
    m.prepare_context(torch.from_numpy(ctx), torch.from_numpy(mask))
    torch.cuda.synchronize()
    el = np.nonzero(key1 >= 0)[0]
    vc = m.debug_buffer('vc', torch.bfloat16, (nb, B, H, Lcp, DV)).float().cpu().numpy()
    v = np.stack([vc[b, el, :, key1[el], :dh].reshape(len(el), D) for b in range(nb)])      # the bf16 value row of every single-key element, per block
    zd = m.debug_buffer('zd', torch.float32, (nb, B, D)).cpu().numpy()
    ref, bound = TE.zd_ref_bound(fx, v)
    assert np.isfinite(zd).all()
    for b in range(nb):
        r = TE.worst_ratio(zd[b, el], ref[b], bound[b])
        record(f'(h) {name} B={B} zd block {b}: worst |got - ref64| / bound {r:.4f}')
        assert r <= 1.0, (b, r)
    assert not zd[:, key1 < 0].any()      # the multi-key elements have no vector
    # the read-back is the kernel's operand only if both kernels round alike: vc (k_headnorm) against the live fp32 ckv, which holds the last block
    Mc, Mcp = B * LC, (B * LC + 127) // 128 * 128
    ckv = m.debug_buffer('ckv', torch.float32, (Mcp, 2 * D)).cpu().numpy()
    assert np.array_equal(TE.bf16r(ckv[el * LC + key1[el], D:]).view(np.uint32), v[nb - 1].view(np.uint32))
    if B != 4:
        return
    # casts: ctx_bf = bf16(ctx), c1b = bf16(silu(c1)), pad columns exactly zero
    Dc = fx.cfg['context_dim']
    ldC = (Dc + 63) // 64 * 64
    ctx_bf = m.debug_buffer('ctx_bf', torch.bfloat16, (Mcp, ldC)).float().cpu().numpy()
    c1 = m.debug_buffer('c1', torch.float32, (Mcp, D)).cpu().numpy()
    c1b = m.debug_buffer('c1b', torch.bfloat16, (Mcp, ldD)).float().cpu().numpy()
    x64 = c1[:Mc].astype(f64)
    for what, got, want, N in (('ctx_bf', ctx_bf, ctx.reshape(Mc, Dc).astype(f64), Dc), ('c1b', c1b, x64 / (1 + np.exp(-x64)), D)):
        r = TE.worst_ratio(got[:Mc, :N], want, TE.bf16_ulp_bound(want))
        record(f'(h) {name} cast {what}: worst |got - ref64| in bf16 ulps {r:.3f}')
        assert r <= 1.0, (what, r)
        assert not got[:Mc, N:].any() and not got[Mc:].any(), what
    assert np.array_equal(ctx_bf[:Mc, :Dc], TE.bf16r(ctx.reshape(Mc, Dc)))      # the identity cast is the rounding itself
    assert ldC > Dc and (ldD > D) == (D % 64 != 0)
