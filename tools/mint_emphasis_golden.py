"""Mint the goldens of prompt emphasis (tests/test_emphasis_gpu.py): tests/golden/forward_emphasis_{xs,xs64}.npz and tests/golden/sampler_emphasis_xs.npz.

    python tools/mint_emphasis_golden.py [--out tests/golden]

A token with integer weight n is the same attention as that token's context row repeated n times, so the UNMODIFIED numpy oracle (oracle.dit.DiTOracle, fp32, itself gated
against the reference goldens) mints the integer set on the duplicated context.  Nothing under oracle/ changes.

  integer set     x and timesteps of the fixtures dit_xs / dit_xs64 (L 96), the first 20 tokens of their context, all valid.  Of the candidate patterns in PATTERNS the one
                  farthest from the unweighted result at the first timestep is kept; the meta records every figure, and the oracle's own floor: the same duplicated context
                  with its rows permuted.
  fractional set  an oracle subclass in this tool that overrides the softmax of every block's CROSS-attention with the bias ln w[b][j] on the score of key j.  It is first
                  held to the integer set: the subclass on the integer weights reproduces the duplicated-context result within 20 times the permuted-rows floor (the
                  subclass adds ln w in fp64 where duplication adds fp32 terms).  Then it mints FRACTIONAL (0.3 ... 12.5 on six of the 20 tokens).
  sampler         the inputs of sampler_smp_xs_e0 (20 steps, guidance 3.5, editing) through the loop of tools/mint_multistep_golden.py with DDIM and DPM-Solver++(2M), the
                  conditional row weighted (fractional weights on its valid tokens), the unconditional row single-key with weight 1.
Condition: every stored weighted result lies at least 5 gates (1e-1 rel-L2) from the unweighted one, which is stored beside it; a host test asserts it on the arrays.
CPU only, a few minutes."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.dit import DiTOracle, layer_norm, linear, merge_heads, split_heads   # noqa: E402

GATE = 2e-2
LT, L = 20, 96
PATTERNS = {'3x8': ([2, 7, 13], 8), '1x16': ([5], 16), '5x4': ([1, 4, 9, 12, 17], 4), '2x6': ([0, 19], 6)}      # name -> (tokens, weight); the others weigh 1
FRACTIONAL = {0: 12.5, 1: 12.5, 6: 0.3, 7: 0.3, 8: 0.3, 15: 1.6}


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rel(x, y):
    return float(np.linalg.norm(np.asarray(x, np.float64) - y) / np.linalg.norm(np.asarray(y, np.float64)))


def weighted_sdpa(q, k, v, key_mask, w):
    """oracle.dit.sdpa with the bias ln w[b][j] on key j; w [B][Lk], read at valid keys only"""
    dh = q.shape[-1]
    s = (q @ k.transpose(0, 1, 3, 2)) * q.dtype.type(dh ** -0.5)
    lw = np.log(np.where(key_mask, w.astype(np.float64), 1.0))[:, None, None, :]
    s = np.where(key_mask[:, None, None, :], s.astype(np.float64) + lw, -np.inf)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return (p @ v.astype(np.float64)).astype(q.dtype)


class EmphasisOracle(DiTOracle):
    """The oracle whose cross-attention weighs the context tokens (tokw None: the parent, unchanged)."""
    tokw = None

    def attention(self, pfx, x, context=None, key_mask=None, rope=None, tap=None):
        if context is None or self.tokw is None:
            return super().attention(pfx, x, context=context, key_mask=key_mask, rope=rope, tap=tap)
        H = self.H
        q = split_heads(linear(x, self.p(f'{pfx}.to_q.weight')), H)
        k = split_heads(linear(context, self.p(f'{pfx}.to_k.weight')), H)
        v = split_heads(linear(context, self.p(f'{pfx}.to_v.weight')), H)
        q = layer_norm(q, self.p(f'{pfx}.norm_q.weight'), self.p(f'{pfx}.norm_q.bias'))
        k = layer_norm(k, self.p(f'{pfx}.norm_k.weight'), self.p(f'{pfx}.norm_k.bias'))
        mask = np.ones(context.shape[:2], bool) if key_mask is None else key_mask
        o = merge_heads(weighted_sdpa(q, k, v, mask, self.tokw))
        return linear(o, self.p(f'{pfx}.proj.weight'), self.p(f'{pfx}.proj.bias'))


def int_weights(pattern, B):
    toks, n = PATTERNS[pattern]
    w = np.ones((B, LT), np.float32)
    w[:, toks] = n
    return w


def frac_weights(B, valid=LT):
    w = np.ones((B, LT), np.float32)
    for j, x in FRACTIONAL.items():
        if j < valid:
            w[:, j] = x
    return w


def duplicated(ctx, w):
    """context rows repeated by their integer weights (the same weights in every batch row) -> (ctx, mask)"""
    rep = np.repeat(np.arange(ctx.shape[1]), w[0].astype(int))
    return ctx[:, rep], np.ones((ctx.shape[0], len(rep)), bool)


def mint_forward(name, out):
    from tests.util import golden_case
    cfg, sd, inp, kw, g, meta = golden_case(name)
    assert not kw and meta['L'] == L, 'a plain forward fixture of 96 frames'
    plain_o, o = DiTOracle(cfg, sd), EmphasisOracle(cfg, sd)
    B = inp['x'].shape[0]
    ctx = np.ascontiguousarray(inp['ctx'][:, :LT]).astype(np.float32)
    msk = np.ones((B, LT), bool)
    t0 = meta['timesteps'][0]
    fwd = lambda c, m, t=t0: plain_o.forward(inp['x'], t, c, m)[0].astype(np.float32)      # noqa: E731

    def run(w, t):
        o.tokw = np.asarray(w, np.float32)
        try:
            return o.forward(inp['x'], t, ctx, msk)[0].astype(np.float32)
        finally:
            o.tokw = None
    plain = fwd(ctx, msk)
    found, floors = {}, {}
    for pat in PATTERNS:
        c, m = duplicated(ctx, int_weights(pat, B))
        y = fwd(c, m)
        perm = np.random.RandomState(7).permutation(c.shape[1])
        found[pat] = rel(y, plain)
        floors[pat] = rel(fwd(c[:, perm], m[:, perm]), y)
        print(f'{name} t={t0}: pattern {pat}: {found[pat]:.3e} from the unweighted result; permuted-rows floor {floors[pat]:.3e}')
    best = max(found, key=found.get)
    print(f'{name}: kept pattern {best}: {found[best]:.3e} (gate {GATE:.0e}, condition {5 * GATE:.0e})')
    assert found[best] >= 5 * GATE, found
    w_int = int_weights(best, B)
    c, m = duplicated(ctx, w_int)
    arrays = dict(ctx=ctx, w_int=w_int, w_frac=frac_weights(B))
    sub = {}
    for t in meta['timesteps']:
        arrays[f'plain_t{t}'] = fwd(ctx, msk, t)
        arrays[f'pred_int_t{t}'] = fwd(c, m, t)
        sub[t] = rel(run(w_int, t), arrays[f'pred_int_t{t}'])
        print(f'{name} t={t}: the subclass on the integer weights vs the duplicated context: rel-L2 {sub[t]:.3e} (margin {20 * floors[best]:.3e})')
        assert sub[t] <= 20 * floors[best], (t, sub[t], floors[best])
        arrays[f'pred_frac_t{t}'] = run(arrays['w_frac'], t)
    frac_away = rel(arrays[f'pred_frac_t{t0}'], plain)
    print(f'{name}: fractional weights: {frac_away:.3e} from the unweighted result')
    assert frac_away >= 5 * GATE, frac_away
    m_ = dict(base='dit_' + name, size=meta['size'], L=L, LT=LT, seed_w=meta['seed_w'], seed_in=meta['seed_in'], timesteps=list(meta['timesteps']), pattern=best,
              int_vs_plain=found[best], frac_vs_plain=frac_away, pattern_search=found, permuted_rows_floor=floors, subclass_vs_duplicated={str(k): v for k, v in sub.items()},
              fractional={str(k): v for k, v in FRACTIONAL.items()})
    path = os.path.join(out, f'forward_emphasis_{name}.npz')
    np.savez_compressed(path, meta=np.array(repr(m_)), **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')


def mint_sampler(out):
    from ezaudio_amd.scheduler import DDIMScheduler
    from tests.util import DIFF, sampler_case
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert meta['eta'] == 0.0 and meta['L'] == L
    loop = _tool('mint_multistep_golden').multistep_loop
    cond, cmask = inp['ctx'][0:1], inp['ctx_mask'][0:1]
    unc, umask = inp['ctx'][1:2], inp['ctx_mask'][1:2]
    Lc, nv = cond.shape[1], int(cmask.sum())
    assert int(umask.sum()) == 1, 'the unconditional row is single-key'
    W = np.ones((1, Lc), np.float32)
    for j, x in FRACTIONAL.items():
        if j < nv:
            W[0, j] = x
    assert bool((W[cmask] != 1).any())
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(meta['steps'])
    ch = sch.multistep_coefficients()
    o = EmphasisOracle(cfg, sd)

    def denoise(x, t, ctx, msk, gt, gm):
        assert ctx.shape[0] == 2      # the loop hands over the CFG pair [conditional, unconditional]
        o.tokw = np.concatenate([W, np.ones((1, Lc), np.float32)], 0)
        return o.forward(x, t, ctx, msk, gt=gt, mae_mask_infer=gm)[0]
    args = (denoise, cond, cmask, unc, umask, init, sch.ddim_coefficients(0))
    kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'],
              gt=inp['gt'][0:1] if meta['with_gt'] else None, gt_mask=inp['gt_mask'][0:1] if meta['with_gt'] else None)
    arrays = dict(weights=W)
    arrays['latent_ddim'] = loop(*args, [0.0] * len(ch), **kw).astype(np.float32)
    arrays['latent_dpmpp_2m'] = loop(*args, ch, **kw).astype(np.float32)
    sep = rel(arrays['latent_ddim'], g['latent'])
    print(f'the weighted loop vs the unweighted golden smp_xs_e0 over {meta["steps"]} steps, DDIM: rel-L2 {sep:.3e} ({nv} valid tokens)')
    m = dict(base='smp_xs_e0', size=meta['size'], L=L, steps=meta['steps'], seed_w=meta['seed_w'], seed_in=meta['seed_in'], n_valid=nv,
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'], weighted_vs_plain_ddim=sep)
    path = os.path.join(out, 'sampler_emphasis_xs.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name in ('xs', 'xs64'):
        mint_forward(name, a.out)
    mint_sampler(a.out)


if __name__ == '__main__':
    main()
