"""T5 encoder timing on the GPU (diagnostic, not a test): the HIP encoder (ezaudio_amd/t5.py) against transformers' T5EncoderModel on
torch eager ops, same GPU, same process, alternating.

    python tools/bench_t5.py [--layers 24] [--rounds 10] [--batches 1,2,8] [--length 100]

flan-t5-xl shape (24 layers, d_model 2048, d_ff 5120, 32 heads of 64) with random weights, the transformers model in fp32 as
EzAudio.load_models loads it.  Each round times a run of `--calls` encodes of one implementation between two HIP events, then the
other; the figure is the median over the rounds of the per-call time, after warm-up.  One `inference()` call encodes twice (prompts,
negative prompts): the last column is 2 x the per-call time.  Prints one JSON line per batch size."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
from ezaudio_amd.build import source_hash   # noqa: E402
from ezaudio_amd.t5 import T5Encoder        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--layers', type=int, default=24)
ap.add_argument('--rounds', type=int, default=10)
ap.add_argument('--calls', type=int, default=5)
ap.add_argument('--batches', default='1,2,8')
ap.add_argument('--length', type=int, default=100)
args = ap.parse_args()

from transformers import T5Config, T5EncoderModel   # noqa: E402

torch.manual_seed(0)
cfg = T5Config(vocab_size=32128, d_model=2048, d_kv=64, num_heads=32, d_ff=5120, num_layers=args.layers, feed_forward_proj='gated-gelu_new',
               is_encoder_decoder=False, use_cache=False)
hf = T5EncoderModel(cfg).eval()
for n, p in hf.named_parameters():   # transformers' initialiser leaves the norms at 1 and the bias table tiny: make both count
    if 'layer_norm' in n:
        p.data.uniform_(0.9, 1.1)
    if 'relative_attention_bias' in n:
        p.data.uniform_(-1, 1)
native = T5Encoder.from_hf(hf, 'cuda')
hf = hf.to('cuda')
L = args.length


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


with torch.no_grad():
    for B in [int(b) for b in args.batches.split(',')]:
        ids = torch.randint(0, 32128, (B, L), device='cuda')
        mask = torch.zeros(B, L, dtype=torch.bool, device='cuda')
        for b in range(B):
            mask[b, :(12 if b % 2 == 0 else 1) if B > 1 else 12] = True   # a prompt / the empty prompt, as make_inputs has them
        f_native = lambda: native(input_ids=ids, attention_mask=mask).last_hidden_state
        f_hf = lambda: hf(input_ids=ids, attention_mask=mask).last_hidden_state
        for _ in range(3):
            y_n, y_h = f_native(), f_hf()
        torch.cuda.synchronize()
        valid = mask.unsqueeze(-1).expand_as(y_h)
        rel = float((y_n[valid] - y_h[valid]).double().norm() / y_h[valid].double().norm())
        tn, th = [], []
        for _ in range(args.rounds):
            tn.append(timed(f_native, args.calls))
            th.append(timed(f_hf, args.calls))
        r = dict(bench='t5_encode', source_hash=source_hash(), layers=args.layers, B=B, L=L, rounds=args.rounds, calls=args.calls,
                 native_ms=round(statistics.median(tn), 4), native_min_ms=round(min(tn), 4), native_max_ms=round(max(tn), 4),
                 hf_ms=round(statistics.median(th), 4), hf_min_ms=round(min(th), 4), hf_max_ms=round(max(th), 4),
                 native_vs_hf_rel_l2=round(rel, 5), per_inference_native_ms=round(2 * statistics.median(tn), 4),
                 per_inference_hf_ms=round(2 * statistics.median(th), 4))
        print(json.dumps(r), flush=True)
