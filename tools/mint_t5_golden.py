"""Mint tests/golden/t5_tiny_{a,b}.npz from transformers' T5EncoderModel (needs `transformers`; the GPU tests then do not).

    python tools/mint_t5_golden.py

For each tiny configuration of tests/t5_ref.py: the model is built in double with the weights of t5_ref.make_weights (seed in the
file), run on B = 3 sequences with (1, 37, L) valid tokens for L = 7, 100, 130, and ids / mask / last_hidden_state (fp32) are
stored.  T5LayerNorm computes its variance in float32 whatever the model's dtype; `double_norm` replaces that one cast so that
the double model is double throughout (tests/test_t5_host.py holds the fp64 judge to 1e-9 of it).
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import t5_ref  # noqa: E402

SEED_W, SEED_IN = 1, 3
LENGTHS = (7, 100, 130)


@contextlib.contextmanager
def double_norm():
    import transformers.models.t5.modeling_t5 as M
    old = M.T5LayerNorm.forward

    def forward(self, x):   # the module's own formula without `.to(torch.float32)` on the variance
        return self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))
    M.T5LayerNorm.forward = forward
    try:
        yield
    finally:
        M.T5LayerNorm.forward = old


def hf_model(cfg, sd):
    from transformers import T5Config, T5EncoderModel
    hf = T5EncoderModel(T5Config(**cfg, is_encoder_decoder=False, use_cache=False)).double().eval()
    hf.load_state_dict({k: torch.tensor(v).double() for k, v in sd.items()}, strict=True)
    return hf


def case_inputs(cfg, L):
    return t5_ref.make_ids(cfg, 3, L, SEED_IN), t5_ref.make_mask(3, L, (1, min(37, L), L))


def run_hf(hf, ids, mask):
    with torch.no_grad(), double_norm():
        return hf(input_ids=torch.tensor(ids), attention_mask=torch.tensor(mask).long()).last_hidden_state.numpy()


def main():
    for name in 'ab':
        cfg = t5_ref.config(name)
        hf = hf_model(cfg, t5_ref.make_weights(cfg, SEED_W))
        out = dict(meta=np.array(repr(dict(config=name, seed_w=SEED_W, seed_in=SEED_IN, lengths=LENGTHS, transformers=__import__('transformers').__version__,
                                            model='T5EncoderModel in double with T5LayerNorm.forward REPLACED (variance kept in float64, not cast to float32: '
                                                  'tools/mint_t5_golden.py double_norm) -- the output of a modified transformers, not of the stock module'))))
        for L in LENGTHS:
            ids, mask = case_inputs(cfg, L)
            out[f'ids_{L}'], out[f'mask_{L}'] = ids.astype(np.int32), mask
            out[f'out_{L}'] = run_hf(hf, ids, mask).astype(np.float32)
        path = os.path.join(ROOT, 'tests', 'golden', f't5_tiny_{name}.npz')
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
