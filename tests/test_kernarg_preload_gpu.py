"""The leading (preloaded) kernel parameters of k_gemm_ks / k_gemm_pp / k_gemm_co on an MI355X (run with -m gpu).

A preload can go wrong in two ways: the launcher and the kernel disagree on the order or the width of a leading parameter, or a replayed graph node serves the values of
another launch.  So every test launches the SAME instantiation twice back to back with different leading values (other operand buffers, other strides, other sizes),
once eagerly and once captured in one graph that is replayed twice with the inputs rewritten in between, and checks every result against float64 of the operands it was
given.  Hooks and gates are those of the kernel-level tests: ezdit_test_gemm (tests/test_gpu.py test_gemm_against_fp32_matmul), also with split-K slabs, and
ezdit_test_consumer (test_consumer_geglu_gemm_finishes_the_layernorm_of_its_operand, tests/kernel_emul.py) for the step counter's address.  The strides' slack is poisoned: a row
fetched at another stride, or rows beyond M, show up as NaN.  (k_attn keeps its one by-value argument: its preload was measured and put back)"""
import ctypes as C

import pytest
import torch

from tests import kernel_emul as KE
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return 'cuda:0'


def _eager_then_graph(launch_all, check_all, rewrite):
    """launch_all(stream) issues the two launches; check_all() synchronises and checks both; rewrite() puts other inputs into the same buffers (and resets the outputs)."""
    launch_all(None)
    check_all()
    rewrite()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch_all(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    g.replay()
    check_all()
    rewrite()
    g.replay()
    check_all()


# ---------------------------------------------------------------------------------------------------
# GEMM families: 70 = k_gemm_ks (48 x 96), 60 / 61 = k_gemm_pp (128 x 288 un-split schedule, 128 x 144 k-split schedule), 66 = k_gemm_co (128 x 144)
# ---------------------------------------------------------------------------------------------------
class _Gemm:
    def __init__(self, dev, M, N, K, lda, seed):
        self.M, self.N, self.K, self.lda, self.dev, self.seed = M, N, K, lda, dev, seed
        Np = (N + 127) // 128 * 128
        self.A = torch.empty(M + 3, lda, dtype=torch.bfloat16, device=dev)      # (rows behind M and the columns [K, lda): poison)
        self.W = torch.empty(Np, K, dtype=torch.bfloat16, device=dev)
        self.bias = torch.empty(N, device=dev)
        self.out = torch.empty(M, N, device=dev)
        self.fill()

    def fill(self):
        g = torch.Generator().manual_seed(self.seed)
        self.seed += 1
        M, N, K = self.M, self.N, self.K
        A = torch.full((M + 3, self.lda), float('nan'), dtype=torch.bfloat16)
        A[:M, :K] = torch.randn(M, K, generator=g).to(torch.bfloat16)
        W = torch.zeros(self.W.shape[0], K, dtype=torch.bfloat16)
        W[:N] = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
        bias = torch.randn(N, generator=g)
        self.ref = A[:M, :K].double() @ W[:N].double().T + bias.double()
        self.A.copy_(A); self.W.copy_(W); self.bias.copy_(bias)
        self.out.fill_(float('nan'))

    def launch(self, lib, tile, stream):
        rc = lib.ezdit_test_gemm(None, tile * 4 + 0, self.A.data_ptr(), self.lda, self.W.data_ptr(), self.K, self.bias.data_ptr(), self.out.data_ptr(), self.N,
                                 self.M, self.N, self.K, 1, stream)
        assert rc == 0, lib.ezdit_last_error()

    def check(self):
        got = self.out.cpu().double()
        err = (got - self.ref).abs().max().item()
        assert err < 2e-3 * max(1.0, self.ref.abs().max().item()), err      # fp32 accumulation of exact bf16 products (test_gemm_against_fp32_matmul)
        assert rel_l2(got.numpy(), self.ref.numpy()) < 1e-5


@pytest.mark.parametrize('K', [64, 192, 1152])
@pytest.mark.parametrize('M', [1, 33, 130])
@pytest.mark.parametrize('tile', [70, 60, 61, 66])
def test_gemm_launched_twice_with_other_leading_values_eagerly_and_from_a_replayed_graph(lib, dev, tile, M, K):
    """N = 100 and 436: ragged against every tile width (96, 144, 288), multiples of 4.  The second launch has other A / W / bias / out buffers, lda = K + 64 and the other N."""
    a = _Gemm(dev, M, 100, K, K, 1000 * tile + 10 * M + K)
    b = _Gemm(dev, M, 436, K, K + 64, 5000 * tile + 10 * M + K)

    def launch_all(stream):
        a.launch(lib, tile, stream)
        b.launch(lib, tile, stream)

    def check_all():
        torch.cuda.synchronize()
        a.check()
        b.check()

    def rewrite():
        a.fill()
        b.fill()

    _eager_then_graph(launch_all, check_all, rewrite)


# ---------------------------------------------------------------------------------------------------
# split-K launches (EPI_PARTIAL) of k_gemm_pp / k_gemm_co: the split count rides in the top byte of the K parameter, two magic numbers in the slot of the step counter's
# address, the K boxes in the packed box word.  (The panel placement is set by the forward only: tests/test_gpu.py test_placement_and_row_kernel_variants_agree.)
# ---------------------------------------------------------------------------------------------------
class _SplitK(_Gemm):
    def __init__(self, dev, M, N, K, lda, splitk, seed):
        self.splitk, self.Mp = splitk, (M + 127) // 128 * 128
        super().__init__(dev, M, N, K, lda, seed)
        self.out = torch.empty(splitk, self.Mp, N, device=dev)
        self.out.fill_(float('nan'))

    def fill(self):
        super().fill()
        self.ref = self.ref - self.bias.cpu().double()      # slabs carry no bias

    def launch(self, lib, tile, stream):
        rc = lib.ezdit_test_gemm(None, tile * 4 + 1, self.A.data_ptr(), self.lda, self.W.data_ptr(), self.K, None, self.out.data_ptr(), self.N,
                                 self.M, self.N, self.K, self.splitk, stream)
        assert rc == 0, lib.ezdit_last_error()

    def check(self):
        got = self.out.cpu().double()[:, :self.M].sum(0)
        err = (got - self.ref).abs().max().item()
        assert err < 2e-3 * max(1.0, self.ref.abs().max().item()), err
        assert rel_l2(got.numpy(), self.ref.numpy()) < 1e-5


@pytest.mark.parametrize('M,K,s1,s2', [(130, 192, 3, 2), (33, 1152, 6, 9), (300, 320, 2, 5)])      # one K tile per split, 3 / 2 tiles per split, uneven splits (5 tiles: 2 + 3; 1 each)
@pytest.mark.parametrize('tile', [60, 61, 62, 66])
def test_split_k_gemm_launched_twice_with_other_split_counts_eagerly_and_from_a_replayed_graph(lib, dev, tile, M, K, s1, s2):
    a = _SplitK(dev, M, 300, K, K, s1, 9000 * tile + M + K)
    b = _SplitK(dev, M, 436, K, K + 64, s2, 7000 * tile + M + K)

    def launch_all(stream):
        a.launch(lib, tile, stream)
        b.launch(lib, tile, stream)

    def check_all():
        torch.cuda.synchronize()
        a.check()
        b.check()

    def rewrite():
        a.fill(); a.out.fill_(float('nan'))
        b.fill(); b.out.fill_(float('nan'))

    _eager_then_graph(launch_all, check_all, rewrite)


# ---------------------------------------------------------------------------------------------------
# the step counter's address (third leading parameter): the GEGLU consumer reads G' / C' of slot *cur_step.  Two launches with their own counters; between the graph's
# replays the tables are rotated by one slot and the counters follow, so that the same references hold only if each launch reads ITS counter's new value
# ---------------------------------------------------------------------------------------------------
class _GegluConsumer:
    def __init__(self, lib, dev, tile, case):
        M, D, zw, inner = case
        self.lib, self.tile, self.M, self.D, self.zw, self.inner = lib, tile, M, D, zw, inner
        self.c = c = KE.geglu_case(M, D, zw, inner, False)
        W, G, Cc, bias = KE.geglu_device_order(c)
        self.N, self.K = 2 * inner, (D + 63) // 64 * 64
        self.wrows = (self.N + 127) // 128 * 128
        A = torch.zeros(M, self.K, dtype=torch.bfloat16); A[:, :D] = c.A
        Wp = torch.zeros(self.wrows, self.K, dtype=torch.bfloat16); Wp[:self.N, :D] = W
        self.G, self.Cc = G.contiguous(), Cc.contiguous()
        self.Ad, self.Wd, self.bd, self.stats = A.to(dev), Wp.to(dev), bias.to(dev), c.stats.to(dev)
        self.Gd, self.Cd = torch.empty_like(self.G, device=dev), torch.empty_like(self.Cc, device=dev)
        self.cur = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = torch.empty((M, inner), dtype=torch.bfloat16, device=dev)
        self.shift = 0
        self.fill()
        self.ra, self.rb = KE.geglu(c.ref_a()), KE.geglu(c.ref_b())

    def fill(self):
        self.Gd.copy_(self.G.roll(self.shift, 0)); self.Cd.copy_(self.Cc.roll(self.shift, 0))
        self.cur.fill_((self.c.cur_step + self.shift) % self.c.nslots)
        self.out.fill_(float('nan'))
        self.shift += 1

    def launch(self, stream):
        c = self.c
        rc = self.lib.ezdit_test_consumer(self.tile, 2, 0, self.Ad.data_ptr(), self.K, self.Wd.data_ptr(), self.K, self.wrows, self.bd.data_ptr(), self.out.data_ptr(), self.inner,
                                          self.M, self.N, self.K, self.stats.data_ptr(), c.rows_alloc, c.zparts, self.D, self.zw, self.Gd.data_ptr(), self.Cd.data_ptr(), self.N, 1e-5,
                                          self.cur.data_ptr(), None, c.rows_per_b, None, None, None, None, None, None, None, None, None, 0, 0, 0, 0, 0, 0, stream)
        assert rc == 0, self.lib.ezdit_last_error()

    def check(self):
        got = self.out.cpu()
        assert torch.isfinite(got.float()).all()
        assert KE.rel_l2(got, self.ra) < KE.GATE_GEGLU_A      # the gates of test_consumer_geglu_gemm_finishes_the_layernorm_of_its_operand
        assert KE.rel_l2(got, self.rb) < KE.GATE_GEGLU_B


@pytest.mark.parametrize('tile', [60, 66])      # k_gemm_pp 128 x 288, k_gemm_co 128 x 144
def test_consumer_gemm_launched_twice_with_other_step_counters_eagerly_and_from_a_replayed_graph(lib, dev, tile):
    a = _GegluConsumer(lib, dev, tile, (300, 576, 96, 584))
    b = _GegluConsumer(lib, dev, tile, (77, 160, 96, 576))

    def launch_all(stream):
        a.launch(stream)
        b.launch(stream)

    def check_all():
        torch.cuda.synchronize()
        a.check()
        b.check()

    def rewrite():
        a.fill()
        b.fill()

    _eager_then_graph(launch_all, check_all, rewrite)
