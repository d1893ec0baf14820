"""VAE decoder / encoder timing on the GPU (diagnostic, not a test): python tools/bench_vae.py [L] [--batch B]

--batch B: the decode and the encode of B samples of L frames as ONE stacked call against the per-sample loop, alternated in one process; the loop is timed twice
per round (before and after the batched form), so the spread between two runs of the same thing stands next to the difference."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from oracle import vae as V            # noqa: E402  (synthetic weights only)
from ezaudio_amd.vae import OobleckDecoder, OobleckEncoder  # noqa: E402

args = sys.argv[1:]
BATCH = 0
if '--batch' in args:
    i = args.index('--batch')
    BATCH = int(args[i + 1])
    del args[i:i + 2]
L = int(args[0]) if args else 250
cfg = dict(V.VAE_DEFAULT)
dec = OobleckDecoder(device='cuda').load_state_dict(V.make_vae_state_dict(cfg, 6))
enc = OobleckEncoder(device='cuda').load_state_dict(V.make_vae_state_dict(cfg, 6, encoder=True))
z = torch.randn(1, 128, L, device='cuda')
wav = torch.randn(1, 1, L * 480, device='cuda') * 0.3


def timeit(fn, n=10):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


if BATCH:
    zb = torch.randn(BATCH, 128, L, device='cuda')
    wb = torch.randn(BATCH, 1, L * 480, device='cuda') * 0.3
    for what, net, x in (('decode', dec, zb), ('encode', enc, wb)):
        def loop():
            return [net(x[b:b + 1]) for b in range(BATCH)]
        rows = []
        for _ in range(5):
            rows.append((timeit(loop, 5), timeit(lambda: net(x), 5), timeit(loop, 5)))
        a, bt, c = (sorted(r[i] for r in rows)[len(rows) // 2] for i in range(3))
        for r in rows:
            print(f'  {what} B={BATCH} L={L}: loop {r[0]:.3f} ms  batched {r[1]:.3f} ms  loop again {r[2]:.3f} ms', flush=True)
        print(f'{what} B={BATCH} L={L} (medians of 5 rounds x 5 calls): loop {a:.3f} ms, batched {bt:.3f} ms, loop again {c:.3f} ms; '
              f'batched / loop {bt / min(a, c):.3f}, loop / loop spread {abs(a - c) / min(a, c):.3f}', flush=True)
    sys.exit(0)

for tile in (6, 9, 13, 25):   # the ids that address convolutions (csrc/gemm.hip: the lockstep kernel); ezvae_gemm refuses every other
    dec.tile = enc.tile = tile
    try:
        td = timeit(lambda: dec(z))
        te = timeit(lambda: enc(wav))
    except Exception as e:  # noqa: BLE001
        print(tile, 'failed', e)
        continue
    print(f'tile {tile}: decode {td:.3f} ms ({dec.flops(L) / td / 1e9:.1f} TFLOP/s)  encode {te:.3f} ms', flush=True)
