"""Mint the goldens of sliding-window self-attention (tests/test_window_gpu.py): tests/golden/forward_window_{xs,xs64}.npz and tests/golden/sampler_window_xs.npz.

    python tools/mint_window_golden.py [--out tests/golden] [--radius 20] [--sampler-radius 8] [--search]

The reference has no such attention, so this is NOT a run of the reference: it is the numpy oracle (oracle.dit.DiTOracle, fp32, itself gated against the reference
goldens) with ONE call overridden in a subclass -- the softmax of every block's SELF-attention runs over the keys j with |i - j| <= radius.  Nothing under oracle/ changes.

  forward   the inputs, weights and timesteps of the existing fixtures dit_xs / dit_xs64 (L 96).  With the band off the subclass must reproduce those fixtures: the distance
            is printed and asserted first.
  sampler   the inputs of the eta = 0 fixture sampler_smp_xs_e0 (xs, L 96, 20 steps, guidance 3.5, editing with gt / gt_mask) through the loop of
            tools/mint_multistep_golden.py, with DDIM (c_hist = 0) and with DPM-Solver++(2M).  The full-attention run of the same loop is computed beside each and the
            rel-L2 between the two goes into the meta (`window_vs_full_*`): it is what separates the feature from its absence, so it must exceed the test's gate of 2e-2;
            the target is ten times the gate.  At L = 96 radius 20 misses the target (1.7e-1: the fixture edits a clip, and the kept frames of gt dilute the
            difference), so the loop fixture takes the radius of 8 .. 32 that maximises it -- 8, the narrowest (2.7e-1; the figure falls steadily with the radius) --
            and the meta keeps the figures of the searched radii (`radius_search`).  --search prints them again.
CPU only, under a minute."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.dit import DiTOracle, apply_rope, layer_norm, linear, merge_heads, split_heads   # noqa: E402

GATE = 2e-2     # the fused-loop gate of tests/test_gpu.py
# windowed vs full attention over the 20 steps of smp_xs_e0, (DDIM, dpmpp_2m) per radius, as --search measured them
SEARCHED = {8: (0.2697, 0.2647), 12: (0.2291, 0.2245), 16: (0.198, 0.1941), 20: (0.1734, 0.1702), 24: (0.1497, 0.1471), 28: (0.1315, 0.1294), 32: (0.1182, 0.1159)}


def band_sdpa(q, k, v, radius):
    """oracle.dit.sdpa over the keys within `radius` frames of each query"""
    dh, L = q.shape[-1], q.shape[2]
    s = (q @ k.transpose(0, 1, 3, 2)) * q.dtype.type(dh ** -0.5)
    i = np.arange(L)
    s = np.where((np.abs(i[:, None] - i[None, :]) <= radius)[None, None], s, -np.inf)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(axis=-1, keepdims=True)
    return p @ v


class WindowOracle(DiTOracle):
    """DiTOracle whose self-attention sees a band of keys (radius None: the parent, unchanged)."""

    def __init__(self, cfg, sd, radius=None, **kw):
        super().__init__(cfg, sd, **kw)
        self.radius = radius

    def attention(self, pfx, x, context=None, key_mask=None, rope=None, tap=None):
        if context is not None or self.radius is None:
            return super().attention(pfx, x, context=context, key_mask=key_mask, rope=rope, tap=tap)
        H = self.H
        q = split_heads(linear(x, self.p(f'{pfx}.to_q.weight')), H)
        k = split_heads(linear(x, self.p(f'{pfx}.to_k.weight')), H)
        v = split_heads(linear(x, self.p(f'{pfx}.to_v.weight')), H)
        q = layer_norm(q, self.p(f'{pfx}.norm_q.weight'), self.p(f'{pfx}.norm_q.bias'))
        k = layer_norm(k, self.p(f'{pfx}.norm_k.weight'), self.p(f'{pfx}.norm_k.bias'))
        if rope is not None:
            cos, sin = rope
            q = apply_rope(q.astype(np.float32), cos, sin).astype(self.dtype)
            k = apply_rope(k.astype(np.float32), cos, sin).astype(self.dtype)
        o = merge_heads(band_sdpa(q, k, v, self.radius))
        return linear(o, self.p(f'{pfx}.proj.weight'), self.p(f'{pfx}.proj.bias'))


def rel(x, y):
    return float(np.linalg.norm(np.asarray(x, np.float64) - y) / np.linalg.norm(np.asarray(y, np.float64)))


def _multistep_loop():
    spec = importlib.util.spec_from_file_location('mint_multistep_golden', os.path.join(ROOT, 'tools', 'mint_multistep_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.multistep_loop


def mint_forward(name, radius, out):
    from tests.util import golden_case
    cfg, sd, inp, kw, g, meta = golden_case(name)
    assert not kw, 'a plain forward fixture'
    plain, win = WindowOracle(cfg, sd), WindowOracle(cfg, sd, radius)
    arrays = {}
    for t in meta['timesteps']:
        d = rel(plain.forward(inp['x'], t, inp['ctx'], inp['ctx_mask'])[0], g[f'pred_t{t}'])
        print(f'{name} t={t}: the subclass with the band off vs the reference golden dit_{name}: rel-L2 {d:.3e}')
        assert d < 2e-4, d      # tests/test_oracle.py's gate for the oracle against the reference
        arrays[f'pred_t{t}'] = win.forward(inp['x'], t, inp['ctx'], inp['ctx_mask'])[0].astype(np.float32)
        print(f'{name} t={t}: radius {radius} vs full attention: rel-L2 {rel(arrays[f"pred_t{t}"], g[f"pred_t{t}"]):.3e}')
    m = dict(base='dit_' + name, radius=radius, size=meta['size'], L=meta['L'], Lc=meta['Lc'], seed_w=meta['seed_w'], seed_in=meta['seed_in'], n_valid=list(meta['n_valid']),
             timesteps=list(meta['timesteps']), window_vs_full={int(t): rel(arrays[f'pred_t{t}'], g[f'pred_t{t}']) for t in meta['timesteps']})
    path = os.path.join(out, f'forward_window_{name}.npz')
    np.savez_compressed(path, meta=np.array(repr(m)), **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes')


def sampler_runs(radius):
    """(DDIM, 2M) final latents of the smp_xs_e0 inputs at `radius` (None: full attention)"""
    from ezaudio_amd.scheduler import DDIMScheduler
    from tests.util import DIFF, sampler_case
    cfg, sd, inp, init, noises, g, meta = sampler_case('smp_xs_e0')
    assert meta['eta'] == 0.0
    o = WindowOracle(cfg, sd, radius)

    def denoise(x, t, ctx, msk, gt, gm):
        return o.forward(x, t, ctx, msk, gt=gt, mae_mask_infer=gm)[0]
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(meta['steps'])
    ch = sch.multistep_coefficients()
    args = (denoise, inp['ctx'][0:1], inp['ctx_mask'][0:1], inp['ctx'][1:2], inp['ctx_mask'][1:2], init, sch.ddim_coefficients(0))
    kw = dict(timesteps=[int(t) for t in sch.timesteps], guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'],
              gt=inp['gt'][0:1] if meta['with_gt'] else None, gt_mask=inp['gt_mask'][0:1] if meta['with_gt'] else None)
    loop = _multistep_loop()
    return loop(*args, [0.0] * len(ch), **kw), loop(*args, ch, **kw), g, meta


def mint_sampler(radius, out, search):
    full_ddim, full_ms, g, meta = sampler_runs(None)
    d = rel(full_ddim, g['latent'])
    print(f'full attention, DDIM, through this loop vs the reference golden smp_xs_e0: rel-L2 {d:.3e}')
    assert d < 2e-4, d
    found = dict(SEARCHED)
    if search:
        found = {}
        for r in range(8, 33, 4):
            a, b, _, _ = sampler_runs(r)
            found[r] = (round(rel(a, full_ddim), 4), round(rel(b, full_ms), 4))
            print(f'radius {r}: windowed vs full attention, DDIM {found[r][0]:.3e}, dpmpp_2m {found[r][1]:.3e}')
    ddim, ms, _, _ = sampler_runs(radius)
    sep = dict(ddim=rel(ddim, full_ddim), dpmpp_2m=rel(ms, full_ms))
    print(f'radius {radius}: windowed vs full attention over {meta["steps"]} steps: DDIM {sep["ddim"]:.3e}, dpmpp_2m {sep["dpmpp_2m"]:.3e} (gate {GATE:.0e}, target {10 * GATE:.0e})')
    assert min(sep.values()) > GATE, sep
    m = dict(base='smp_xs_e0', radius=radius, size=meta['size'], L=meta['L'], Lc=meta['Lc'], steps=meta['steps'], seed_w=meta['seed_w'], seed_in=meta['seed_in'],
             guidance_scale=meta['guidance_scale'], guidance_rescale=meta['guidance_rescale'], eta=0.0, with_gt=meta['with_gt'], window_vs_full_ddim=sep['ddim'],
             window_vs_full_dpmpp_2m=sep['dpmpp_2m'], target_met=bool(min(sep.values()) >= 10 * GATE), radius_search=found)
    path = os.path.join(out, 'sampler_window_xs.npz')
    np.savez_compressed(path, latent_ddim=ddim.astype(np.float32), latent_dpmpp_2m=ms.astype(np.float32), meta=np.array(repr(m)))
    print('wrote', path, os.path.getsize(path), 'bytes')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    ap.add_argument('--radius', type=int, default=20)
    ap.add_argument('--sampler-radius', type=int, default=8)
    ap.add_argument('--search', action='store_true')
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for name in ('xs', 'xs64'):
        mint_forward(name, a.radius, a.out)
    mint_sampler(a.sampler_radius, a.out, a.search)


if __name__ == '__main__':
    main()
