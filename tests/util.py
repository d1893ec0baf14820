"""Shared helpers for the parity tests (test infrastructure; may import oracle/)."""
import ast
import os

import numpy as np

from oracle.weights import make_inputs, make_state_dict, model_config, uniform_pm1

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_PARITY = {'path': None}


def record(line):
    """Print a measured parity number and append it to the parity log of this test session: $EZ_PARITY_LOG, default
    gpurun_out/parity_<source hash>.txt (the file the builder copies to profiles/r05_parity.txt: VERDICT r04 item 6 -- every fixture's
    measured rel-L2 / max-abs on the tree that produced it, not only pass / fail dots)."""
    print(line)
    if _PARITY['path'] is None:
        from ezaudio_amd.build import source_hash
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        default = os.path.join(root, 'gpurun_out', 'parity_%s.txt' % source_hash())
        _PARITY['path'] = os.environ.get('EZ_PARITY_LOG', default)
        try:
            os.makedirs(os.path.dirname(_PARITY['path']), exist_ok=True)
        except OSError:
            _PARITY['path'] = ''
    if _PARITY['path']:
        test = os.environ.get('PYTEST_CURRENT_TEST', '').split(' ')[0]
        with open(_PARITY['path'], 'a') as f:
            f.write(f'{test}\t{line}\n')


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = ast.literal_eval(str(g['meta']))
    return g, meta


def golden_case(name):
    """(cfg, state_dict, inputs, extra kwargs for forward, golden arrays, meta) of a dit_* fixture."""
    g, meta = load_golden('dit_' + name)
    cfg = model_config(meta['size'])
    sd = make_state_dict(cfg, meta['seed_w'])
    inp = make_inputs(cfg, B=meta.get('B', 2), L=meta['L'], Lc=meta['Lc'], n_valid=tuple(meta['n_valid']), seed=meta['seed_in'],
                      with_gt=meta['with_gt'])
    kw = {}
    if meta['with_gt']:
        kw = dict(gt=inp['gt'], mae_mask_infer=inp['gt_mask'])
    if meta['cn_skips']:
        D, L = cfg['embed_dim'], meta['L']
        kw['controlnet_skips'] = [(0.1 * uniform_pm1(f'in.cn{i}', 2 * L * D, meta['seed_in'])).reshape(2, L, D)
                                  for i in range(cfg['depth'] // 2)]
    return cfg, sd, inp, kw, g, meta


def sampler_case(name):
    g, meta = load_golden('sampler_' + name)
    cfg = model_config(meta['size'])
    sd = make_state_dict(cfg, meta['seed_w'])
    L, Lc, steps = meta['L'], meta['Lc'], meta['steps']
    inp = make_inputs(cfg, B=2, L=L, Lc=Lc, seed=meta['seed_in'], with_gt=meta['with_gt'])
    C = cfg['out_chans']
    s3 = np.float32(np.sqrt(3.0))
    init = (uniform_pm1('smp.init', C * L, meta['seed_in']) * s3).reshape(1, C, L)
    noises = [(uniform_pm1(f'smp.z{i}', C * L, meta['seed_in']) * s3).reshape(1, C, L) for i in range(steps)]
    return cfg, sd, inp, init, noises, g, meta


def sampler_prompts_case(name):
    """(cfg, per-prompt inputs, golden arrays, meta) of a multi-prompt sampler fixture (oracle/mint_golden.py mint_sampler_prompts): prompt p's inputs are
    dict(ctx [2, Lc, Dc] = (text, negative text), mask [2, Lc], init [1, C, L], noises = steps x [1, C, L]), its golden latent g['latent'][p].  (No state
    dict: the GPU tests' model cache builds its own, and at XL width one costs tens of seconds of CPU.)"""
    from oracle.mint_golden import sampler_prompt_inputs
    g, meta = load_golden('sampler_' + name)
    cfg = model_config(meta['size'])
    prompts = []
    for pr in meta['prompts']:
        ctx, mask, init, noises = sampler_prompt_inputs(cfg, meta['L'], meta['Lc'], meta['steps'], pr)
        prompts.append(dict(ctx=ctx, mask=mask, init=init, noises=noises))
    return cfg, prompts, g, meta


DIFF = dict(num_train_timesteps=1000, beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012,
            prediction_type='v_prediction', rescale_betas_zero_snr=True, timestep_spacing='trailing',
            clip_sample=False)
