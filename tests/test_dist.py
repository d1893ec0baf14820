"""CPU tests of the N > 1 path: world_size 2 over gloo (no GPU needed).  The sharding must be placement-independent:
sharded result == single-process result, bitwise (no cross-sample math exists on the path)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ezaudio_amd.dist import gather_samples, sample_sharded, shard_range


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_sample(start, end, C=4, L=16, seed=2024, steps=3):
    """Stand-in for the GPU sampler with the SAME RNG discipline as ezaudio_amd.sampler.draw_noises:
    one generator per sample, seeded seed + global index, init noise first then one draw per step."""
    from ezaudio_amd.sampler import draw_noises
    outs = []
    for i in range(start, end):
        init, step = draw_noises(C, L, steps, 1.0, seed + i, 'cpu', n_prompts=1)
        outs.append(init[0] * 0.5 + step.sum(dim=0)[0])
    return torch.stack(outs) if outs else torch.zeros(0, C, L)


def _worker(rank, world, port, n_prompts, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out = sample_sharded(_fake_sample, n_prompts)
        q.put((rank, out.clone()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('n_prompts', [5, 2, 1])
def test_sharded_equals_single_process_gloo_world2(n_prompts):
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_prompts, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _fake_sample(0, n_prompts)
    for r in range(world):
        assert torch.equal(results[r], ref)       # every rank holds the full, identical, placement-independent result


def test_shard_range_partitions_everything():
    for n in (0, 1, 7, 8, 32, 33):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [e - s for s, e in spans]
            assert max(sizes) - min(sizes) <= 1


def test_gather_is_identity_without_process_group():
    x = torch.arange(12.).reshape(3, 4)
    assert gather_samples(x, 3) is x


def test_draw_noises_matches_reference_draw_order():
    """Batch-1 call: init noise then one randn per step from ONE generator (src/inference.py:58-67 + scheduler.step)."""
    from ezaudio_amd.sampler import draw_noises
    init, step = draw_noises(3, 5, 4, 1.0, 7, 'cpu')
    g = torch.Generator().manual_seed(7)
    assert torch.equal(init, torch.randn((1, 3, 5), generator=g))
    for i in range(4):
        assert torch.equal(step[i], torch.randn((1, 3, 5), generator=g))
    init0, step0 = draw_noises(3, 5, 4, 0.0, 7, 'cpu')
    assert torch.equal(init0, init) and step0 is None


# ----------------------------------------------------------------------------------------------------------------------
# inference(): prompt sharding + per-rank VAE decode + one all-gather of the waveforms.
# The HIP sampler is replaced by a CPU stand-in that only exercises the host logic: slicing of prompts / negative prompts /
# per-prompt tensors, global per-sample seeds, gather order.
# ----------------------------------------------------------------------------------------------------------------------
class _CpuSampler:
    def __init__(self, unet, scheduler):
        pass

    def prepare(self, text, text_mask, uncond, uncond_mask, init, step_noises, gs, gr, steps, eta, gt=None, gt_mask=None,
                controlnet=None, condition=None, conditioning_scale=1.0):
        # a deterministic function of everything that is per-prompt: prompt embedding, negative embedding, both noise streams
        self.lat = init + 0.1 * step_noises.sum(dim=0) + text.mean(dim=(1, 2))[:, None, None] + 3 * uncond.mean(dim=(1, 2))[:, None, None]
        if condition is not None:
            self.lat = self.lat + condition.mean(dim=(1, 2))[:, None, None]

    def run(self, use_graph=True):
        pass

    def finish(self):
        return self.lat


class _Tok:
    def __call__(self, texts, max_length, padding, truncation, return_tensors):
        ids = torch.tensor([[len(t) + 1, (sum(map(ord, t)) % 50) + 1] + [0] * (max_length - 2) for t in texts])
        return type('B', (), dict(input_ids=ids, attention_mask=(ids > 0).long()))()


def _enc(input_ids, attention_mask):
    return type('O', (), dict(last_hidden_state=torch.sin(input_ids.float())[:, :, None].repeat(1, 1, 6)))()


class _Unet:
    def eval(self):
        return self


PROMPTS = ['a dog barking', 'rain', 'a car passing by on a wet road', 'birds', 'applause']
NEGS = ['noise', '', 'music', 'low quality', 'speech']


def _run_inference(prompts, negs, cond):
    from ezaudio_amd import sampler as S
    S.LatentSampler = _CpuSampler
    params = {'text_encoder': {'max_length': 8}, 'model': {'out_chans': 4}, 'autoencoder': {'scale': 1.0, 'shift': 0.0, 'sr': 80, 'latent_sr': 10}}
    return S.inference(lambda embedding: embedding.repeat_interleave(8, dim=2)[:, :1], _Unet(), None, None, _Tok(), _enc, params, None,
                       prompts, negs, audio_frames=16, guidance_scale=5, ddim_steps=3, eta=1, random_seed=11, device='cpu',
                       condition=cond)


def _inference_worker(rank, world, port, n, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        cond = torch.arange(n * 2 * 5, dtype=torch.float32).reshape(n, 2, 5)
        out = _run_inference(PROMPTS[:n], NEGS[:n], cond)
        q.put((rank, out.clone()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('n', [5, 1])
def test_inference_shards_prompts_and_gathers_audio_gloo_world2(n):
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_inference_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cond = torch.arange(n * 2 * 5, dtype=torch.float32).reshape(n, 2, 5)
    ref = _run_inference(PROMPTS[:n], NEGS[:n], cond)          # no process group here: the unsharded path
    assert ref.shape == (n, 1, 128)
    singles = torch.cat([_run_inference([PROMPTS[i]], [NEGS[i]], cond[i:i + 1]) for i in range(n)]) if n > 1 else ref
    for r in range(world):
        assert torch.equal(results[r], ref)
    # and the batched call is NOT the same as n single calls with the same seed: sample i uses seed + i
    if n > 1:
        assert torch.equal(singles[0], ref[0]) and not torch.equal(singles[1], ref[1])


def _bench_dump(root, env, extra, path):
    """Run bench.py with `extra` arguments, saving the gathered final latents to `path`; returns (json line, latents)."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '20', '--warmup', '10', '--no-cpu-baseline', '--no-probe',
                        '--dump-latents', path] + extra, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), torch.load(path)


def _assert_placement_independent(root, env, multi, size_args, tmp_path):
    """Sample r of the 2-rank job (rank r's prompt, gathered by the collective) == the same prompt run alone in one process."""
    assert multi.shape[0] == 2
    for r in range(2):
        _, single = _bench_dump(root, env, ['--gpus', '1', '--as-rank', str(r)] + size_args, str(tmp_path / f'single{r}.pt'))
        assert single.shape[0] == 1 and torch.equal(single[0], multi[r]), f'rank {r}: gathered latents differ from the single-process run'


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run times exactly --steps steps, prints the headline keys without the --full extras, and --dump-outputs writes the
    latents the timed loop handed back (the same tensor --dump-latents saves) as float32."""
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    res, lat = _bench_dump(root, env, ['--gpus', '1', '--size', 'l', '--steps', '7', '--warmup', '2', '--dump-outputs', str(tmp_path / 'out')],
                           str(tmp_path / 'lat.pt'))
    assert res['steps'] == 7 and res['warmup'] == 2 and res['ms_per_step'] > 0 and res['value'] > 0
    assert {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'} <= set(res)
    assert 'cpu_baseline' not in res and 'config4_shard' not in res and 'dominant_kernel' not in res['roofline']
    dumped = np.load(tmp_path / 'out' / 'latents.npy')
    assert dumped.dtype == np.float32 and np.array_equal(dumped, lat.numpy())


@pytest.mark.gpu
def test_bench_spawns_two_rccl_ranks_when_two_gpus_are_present(tmp_path):
    """`python bench.py --gpus 2` -- the form the driver uses -- must start its own ranks (torch.distributed.run on 127.0.0.1),
    shard the prompts, all-gather over RCCL and print ONE JSON line.  Needs >= 2 GPUs (skipped on the 1-GPU test boxes)."""
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    res, multi = _bench_dump(root, env, ['--gpus', '2'], str(tmp_path / 'multi.pt'))
    assert res['n_gpus'] == 2 and res['distributed']['world_size'] == 2 and res['distributed']['backend'] == 'nccl'
    assert res['scaling'] == 'weak' and res['value'] > 0
    # placement independence over RCCL: what rank r computed on its own GPU and the all-gather delivered is bitwise what one process computes
    _assert_placement_independent(root, env, multi, [], tmp_path)


@pytest.mark.gpu
def test_bench_multi_rank_path_on_one_gpu_over_gloo(tmp_path):
    """The whole N > 1 path of bench.py -- self re-launch under torch.distributed.run on 127.0.0.1, prompt sharding, the timed loop on
    every rank, the final gather, max-over-ranks timing, ONE JSON line from rank 0 -- exercised on a 1-GPU box: both ranks share
    cuda:0 and the collectives go through gloo (RCCL refuses two ranks on one device; the nccl form is the test above)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    res, multi = _bench_dump(root, env, ['--gpus', '2', '--size', 'l', '--dist-backend', 'gloo', '--shared-device'], str(tmp_path / 'multi.pt'))
    assert res['n_gpus'] == 2 and res['distributed']['world_size'] == 2 and res['distributed']['backend'] == 'gloo'
    assert res['scaling'] == 'weak' and res['value'] > 0 and res['config']['prompts_per_gpu'] == 1
    _assert_placement_independent(root, env, multi, ['--size', 'l'], tmp_path)
