"""Mint the goldens of the prompt timeline (tests/test_timeline_gpu.py): tests/golden/forward_timeline_{xs,xs64}.npz and tests/golden/sampler_timeline_xs.npz.

    python tools/mint_timeline_golden.py [--out tests/golden] [--search]

The reference has no such attention, so this is NOT a run of the reference: it is the numpy oracle (oracle.dit.DiTOracle, fp32, itself gated against the reference
goldens) with ONE call overridden in a subclass -- the softmax of every block's CROSS-attention takes the bias ln w[b][s][i] on the scores of prompt s (the keys
[128 s, 128 s + 128) of the context) for query frame i, and a weight of 0 removes the prompt for that frame.  Nothing under oracle/ changes.  The subclass derives from the
windowed oracle of tools/mint_window_golden.py, so the loop can run under a sliding window as well.

  forward   x, weights and timesteps of the fixtures dit_xs / dit_xs64 (L 96); S = 3 prompts of 20 tokens (prompt 0: the fixture's own first 20 tokens, prompts 1 and 2 drawn
            like them from other seeds), all valid.  With one prompt (no weights) the subclass must reproduce those fixtures: the distance is printed and asserted first.
            The scene is a switch 0 -> 1 at frame `a` and a linear cross-fade 1 -> 2 over [b, b + n): of the candidates in SCENES the one is kept whose result is farthest from
            the NEAREST of the three single-prompt results (`scene_vs_single`); the target is ten times the test's gate of 2e-2.  The meta keeps every searched figure.
            A second set of arrays (`ragged_p{p}`) holds the three samples of the padded-batch test: lengths (96, 80, 33), S_i = (3, 1, 2), each run alone at its own length.
  sampler   the inputs of sampler_smp_xs_e0 (20 steps, guidance 3.5, editing) through the loop of tools/mint_multistep_golden.py with DDIM and DPM-Solver++(2M), the
            conditional row under the scene, the unconditional row on its own tokens in prompt 0 with weight (1, 0, 0); again under a window of radius 8.
CPU only, a few minutes."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.dit import layer_norm, linear, merge_heads, split_heads   # noqa: E402
from oracle.weights import make_inputs   # noqa: E402

GATE = 2e-2
SEG, LT, S, L = 128, 20, 3, 96
SCENES = [(30, 50, 30), (24, 48, 24), (32, 64, 16), (20, 40, 40)]      # (switch frame, fade start, fade length)
RAGGED = ((96, 3), (80, 1), (33, 2))                                     # (length, prompts) of the padded-batch samples


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


WindowOracle = _tool('mint_window_golden').WindowOracle


def rel(x, y):
    return float(np.linalg.norm(np.asarray(x, np.float64) - y) / np.linalg.norm(np.asarray(y, np.float64)))


def scene(a, b, n, frames=L):
    """[S][frames]: prompt 0 before frame a, prompt 1 from a on, cross-fading linearly into prompt 2 over [b, b + n)"""
    i = np.arange(frames, dtype=np.float64)
    f = np.clip((i - b + 0.5) / n, 0.0, 1.0)
    return np.stack([(i < a) * 1.0, (i >= a) * (1 - f), (i >= a) * f]).astype(np.float32)


def timeline_sdpa(q, k, v, key_mask, w):
    """oracle.dit.sdpa with the bias ln w[b][s][i] on the keys of prompt s; w [B][S][Lq]"""
    dh = q.shape[-1]
    s = (q @ k.transpose(0, 1, 3, 2)) * q.dtype.type(dh ** -0.5)
    wk = np.repeat(w.astype(np.float64), SEG, axis=1).transpose(0, 2, 1)[:, None]      # [B][1][Lq][Lk]
    ok = (wk > 0) & key_mask[:, None, None, :]
    s = np.where(ok, s.astype(np.float64) + np.log(np.where(wk > 0, wk, 1.0)), -np.inf)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return (p @ v.astype(np.float64)).astype(q.dtype)


class TimelineOracle(WindowOracle):
    """The (windowed) oracle whose cross-attention weights the prompts of the context per frame (tlw None: the parent, unchanged)."""
    tlw = None

    def attention(self, pfx, x, context=None, key_mask=None, rope=None, tap=None):
        if context is None or self.tlw is None:
            return super().attention(pfx, x, context=context, key_mask=key_mask, rope=rope, tap=tap)
        H = self.H
        q = split_heads(linear(x, self.p(f'{pfx}.to_q.weight')), H)
        k = split_heads(linear(context, self.p(f'{pfx}.to_k.weight')), H)
        v = split_heads(linear(context, self.p(f'{pfx}.to_v.weight')), H)
        q = layer_norm(q, self.p(f'{pfx}.norm_q.weight'), self.p(f'{pfx}.norm_q.bias'))
        k = layer_norm(k, self.p(f'{pfx}.norm_k.weight'), self.p(f'{pfx}.norm_k.bias'))
        o = merge_heads(timeline_sdpa(q, k, v, key_mask, self.tlw))
        return linear(o, self.p(f'{pfx}.proj.weight'), self.p(f'{pfx}.proj.bias'))


def prompts_of(cfg, ctx0, seed, B):
    """(ctx [B][S][LT][Dc], mask [B][S][LT]): prompt 0 = the first LT tokens of ctx0, prompts 1, 2 drawn from seeds seed + 101 s"""
    rows = [np.asarray(ctx0)[:, :LT]]
    for s in range(1, S):
        rows.append(make_inputs(cfg, B=B, L=L, Lc=LT, n_valid=(LT,) * B, seed=seed + 101 * s, with_gt=False)['ctx'][:, :LT])
    return np.stack(rows, 1).astype(np.float32), np.ones((B, S, LT), dtype=bool)


def aligned(ctx, mask):
    """[B][S][LT][Dc], [B][S][LT] -> [B][128 S][Dc], [B][128 S] (sampler.timeline_context)"""
    B, n = ctx.shape[0], ctx.shape[1]
    c = np.zeros((B, n, SEG, ctx.shape[-1]), np.float32)
    m = np.zeros((B, n, SEG), bool)
    c[:, :, :ctx.shape[2]] = ctx
    m[:, :, :ctx.shape[2]] = mask
    return c.reshape(B, n * SEG, -1), m.reshape(B, n * SEG)


def mint_forward(name, out, search):
    from tests.util import golden_case
    cfg, sd, inp, kw, g, meta = golden_case(name)
    assert not kw and meta['L'] == L, 'a plain forward fixture of 96 frames'
    o = TimelineOracle(cfg, sd)
    B = inp['x'].shape[0]
    ctx4, msk4 = prompts_of(cfg, inp['ctx'], meta['seed_in'], B)
    ctx, msk = aligned(ctx4, msk4)
    t0 = meta['timesteps'][0]
    d = rel(o.forward(inp['x'], t0, inp['ctx'], inp['ctx_mask'])[0], g[f'pred_t{t0}'])
    print(f'{name} t={t0}: the subclass without a timeline vs the reference golden dit_{name}: rel-L2 {d:.3e}')
    assert d < 2e-4, d

    def run(w, t, x=inp['x'], c=ctx, m=msk):
        o.tlw = np.asarray(w, np.float32)
        try:
            return o.forward(x, t, c, m)[0].astype(np.float32)
        finally:
            o.tlw = None
    one = np.zeros((B, S, L), np.float32)
    singles = []
    for s in range(S):
        w = one.copy(); w[:, s] = 1
        singles.append(run(w, t0))
    c1, m1 = aligned(ctx4[:, :1], msk4[:, :1])
    d1 = rel(run(np.ones((B, 1, L)), t0, c=c1, m=m1), o.forward(inp['x'], t0, c1, m1)[0])
    print(f'{name}: S = 1 with weight 1 vs the subclass without a timeline on the same context: rel-L2 {d1:.3e}')
    assert d1 < 1e-6, d1
    found = {}
    for sc in SCENES:
        w = np.broadcast_to(scene(*sc), (B, S, L))
        y = run(w, t0)
        found[sc] = round(min(rel(y, s_) for s_ in singles), 4)
        print(f'{name}: scene {sc}: distance to the nearest single-prompt result {found[sc]:.3e}')
    best = max(found, key=found.get)
    print(f'{name}: kept scene {best}: {found[best]:.3e} (gate {GATE:.0e}, target {10 * GATE:.0e})')
    assert found[best] > GATE, found
    W = np.broadcast_to(scene(*best), (B, S, L)).copy()
    arrays = dict(ctx=ctx4, weights=W)
    for t in meta['timesteps']:
        arrays[f'pred_t{t}'] = run(W, t)
    vs = [rel(arrays[f'pred_t{t0}'], s_) for s_ in singles]
    # the padded batch: sample p = row 0's x cut to its length, its first S_p prompts, the scene scaled to its length; alone, at its own length
    for p, (n, sp) in enumerate(RAGGED):
        a_, b_, n_ = [max(1, round(v * n / L)) for v in best]
        wp = {3: scene(a_, b_, n_, frames=n), 2: scene(a_, 10 ** 6, 1, frames=n)[:2], 1: np.ones((1, n), np.float32)}[sp]      # two prompts: the switch alone
        cp, mp = aligned(ctx4[0:1, :sp], msk4[0:1, :sp])
        arrays[f'ragged_w{p}'] = wp.astype(np.float32)
        arrays[f'ragged_p{p}'] = run(wp[None], t0, x=inp['x'][0:1, :, :n], c=cp, m=mp)
    m = dict(base='dit_' + name, size=meta['size'], L=L, S=S, LT=LT, seed_w=meta['seed_w'], seed_in=meta['seed_in'], timesteps=list(meta['timesteps']), scene=list(best),
             scene_vs_single=vs, target_met=bool(min(vs) >= 10 * GATE), scene_search={str(k): v for k, v in found.items()}, ragged=[list(r) for r in RAGGED])
    path = os.path.join(out, f'forward_timeline_{name}.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')
    return best


def mint_sampler(best, out):
    from ezaudio_amd.scheduler import DDIMScheduler
    from tests.util import DIFF, sampler_case
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert meta['eta'] == 0.0 and meta['L'] == L
    loop = _tool('mint_multistep_golden').multistep_loop
    ctx4, msk4 = prompts_of(cfg, inp['ctx'][0:1], meta['seed_in'], 1)
    cond, cmask = aligned(ctx4, msk4)
    lu = min(inp['ctx'].shape[1], SEG)
    unc, umask = aligned(inp['ctx'][1:2, None, :lu], inp['ctx_mask'][1:2, None, :lu])
    unc = np.concatenate([unc, np.zeros((1, (S - 1) * SEG, unc.shape[-1]), np.float32)], 1)
    umask = np.concatenate([umask, np.zeros((1, (S - 1) * SEG), bool)], 1)
    W = scene(*best)[None]
    W0 = np.zeros((1, S, L), np.float32); W0[:, 0] = 1
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(meta['steps'])
    ch = sch.multistep_coefficients()
    arrays, sep = dict(ctx=ctx4, weights=W), {}
    for radius in (None, 8):
        o = TimelineOracle(cfg, sd, radius)

        def denoise(x, t, ctx, msk, gt, gm):
            assert ctx.shape[0] == 2      # the loop hands over the CFG pair [conditional, unconditional]
            o.tlw = np.concatenate([W, W0], 0)
            return o.forward(x, t, ctx, msk, gt=gt, mae_mask_infer=gm)[0]
        args = (denoise, cond, cmask, unc, umask, init, sch.ddim_coefficients(0))
        kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'],
                  gt=inp['gt'][0:1] if meta['with_gt'] else None, gt_mask=inp['gt_mask'][0:1] if meta['with_gt'] else None)
        tag = '' if radius is None else f'_r{radius}'
        arrays['latent_ddim' + tag] = loop(*args, [0.0] * len(ch), **kw).astype(np.float32)
        arrays['latent_dpmpp_2m' + tag] = loop(*args, ch, **kw).astype(np.float32)
        if radius is None:
            sep = dict(ddim=rel(arrays['latent_ddim'], g['latent']))
            print(f'the scene vs the one-prompt golden smp_xs_e0 over {meta["steps"]} steps, DDIM: rel-L2 {sep["ddim"]:.3e}')
    m = dict(base='smp_xs_e0', size=meta['size'], L=L, S=S, LT=LT, steps=meta['steps'], seed_w=meta['seed_w'], seed_in=meta['seed_in'], scene=list(best), radius=8,
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'], scene_vs_plain_ddim=sep['ddim'])
    path = os.path.join(out, 'sampler_timeline_xs.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--search', action='store_true', help='(the scenes of SCENES are always searched; kept for symmetry with the other minting tools)')
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    best = None
    for name in ('xs', 'xs64'):
        b = mint_forward(name, a.out, a.search)
        best = best or b
    mint_sampler(best, a.out)


if __name__ == '__main__':
    main()
