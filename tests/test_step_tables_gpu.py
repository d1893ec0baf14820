"""GPU tests of the run-time tables of the fused sampler step as a group (include/ezdit.h, "Run-time tables of the step"): lengths, pair lengths, ControlNet
scales, sample settings, multistep, start and canvas.

1. The captured step is kept while a table that is on takes new values and dropped exactly when a table is switched on or off (or a kernel argument next to
   it changes).  A capture is observed through the diagnostic option `trace_launches`: capturing the step prints its launches to stderr, a replay of the
   captured graph prints nothing.
2. Binding the workspace again ends the sampler call: the run and the call-scoped setters answer EZDIT_E_STATE until ezdit_sampler_begin.

xs width, the inputs of smp_xs_e0 (20 steps, L = 96) under two or three prompts: the helpers of tests/test_canvas_gpu.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.weights import uniform_pm1
from tests.test_canvas_gpu import A_OFFS, _arr, _case, _finish, _prepare
from tests.test_sample_params_gpu import get_model, t_
from tests.test_start_gpu import _scheduler

pytestmark = pytest.mark.gpu

K = 20
TWO = [0, 96]   # two windows that share no frame, without a canvas: the plain call of two prompts


class _Watch:
    """run(1, use_graph=True) of a prepared call, and whether the step was captured for it."""

    def __init__(self, lib, capfd, smp):
        self.lib, self.capfd, self.smp, self.m = lib, capfd, smp, get_model('xs', 1)
        self.st = C.c_void_p(smp.stream.cuda_stream)
        assert lib.ezdit_set_option(self.m._h, b'trace_launches', 1) == 0

    def captured(self):
        self.capfd.readouterr()
        self.smp.run(1, use_graph=True)
        self.smp.stream.synchronize()
        err = self.capfd.readouterr().err
        assert torch.isfinite(self.smp.latents).all()
        return 'launch ' in err

    def check(self, steps):
        """steps: (what, callable that changes a table or None, whether the next run captures)"""
        for what, change, capture in steps:
            if change is not None:
                with torch.cuda.stream(self.smp.stream):
                    rc = change()
                assert rc in (None, 0), (what, self.lib.ezdit_last_error())
            assert self.captured() == capture, what

    def close(self):
        assert self.lib.ezdit_set_option(self.m._h, b'trace_launches', 0) == 0


@pytest.fixture
def watch(lib, capfd):
    made = []

    def make(smp):
        made.append(_Watch(lib, capfd, smp))
        return made[-1]
    yield make
    for w in made:
        w.close()


def test_new_lengths_keep_the_graph_on_and_off_drop_it(lib, watch):
    m = get_model('xs', 1)
    w = watch(_prepare(TWO))
    try:
        w.check([('first run', None, True),
                 ('on', lambda: m.set_lengths([96, 80], w.st), True),
                 ('new lengths', lambda: m.set_lengths([70, 96], w.st), False),
                 ('off', lambda: m.set_lengths(None, w.st), True),
                 ('off again', lambda: m.set_lengths(None, w.st), False)])
    finally:
        m.set_lengths(None)


def test_new_sample_params_keep_the_graph_on_and_off_drop_it(lib, watch):
    w = watch(_prepare(TWO))
    w.check([('first run', None, True),
             ('on', lambda: w.smp.set_sample_params([3.5, 2.0], [0.5, 0.0], [0.0, 0.0]), True),
             ('new values', lambda: w.smp.set_sample_params([1.5, 4.0], [0.0, 0.3], [0.0, 0.0]), False),
             ('off', lambda: w.smp.set_sample_params(), True)])


def test_new_multistep_coefficients_keep_the_graph_another_history_drops_it(lib, watch):
    w = watch(_prepare(TWO))
    m = w.m
    h1, h2 = torch.zeros_like(w.smp.latents), torch.zeros_like(w.smp.latents)
    ch = _scheduler(K).multistep_coefficients()
    set_ = lambda c, hist: lib.ezdit_sampler_set_multistep(m._h, None if c is None else (C.c_float * K)(*c), K, None if hist is None else hist.data_ptr(), w.st)   # noqa: E731
    w.check([('first run', None, True),
             ('on', lambda: set_(ch, h1), True),
             ('new c_hist, the same history', lambda: set_([0.5 * v for v in ch], h1), False),
             ('another history tensor', lambda: set_(ch, h2), True),
             ('off', lambda: set_(None, None), True)])


def test_new_starts_keep_the_graph_on_and_off_drop_it(lib, watch):
    w = watch(_prepare(TWO))
    set_ = lambda v: lib.ezdit_sampler_set_start(w.m._h, None if v is None else _arr(v), 0 if v is None else 2, w.st)   # noqa: E731
    w.check([('first run', None, True),
             ('on', lambda: set_([0, 3]), True),
             ('other starts', lambda: set_([5, 2]), False),
             ('off', lambda: set_(None), True)])


def test_new_canvas_offsets_keep_the_graph_another_ramp_drops_it(lib, watch):
    w = watch(_prepare(A_OFFS))
    w.check([('first run', None, True),
             ('on', lambda: w.smp.set_canvas(A_OFFS, 200, 44), True),
             ('new offsets, the same T and ramp', lambda: w.smp.set_canvas([0, 50, 104], 200, 44), False),
             ('another ramp', lambda: w.smp.set_canvas([0, 50, 104], 200, 20), True),
             ('off', lambda: w.smp.set_canvas(), True)])


def _controlnet():
    from ezaudio_amd import DiTControlNet
    from oracle.controlnet import CN_DEFAULT, make_controlnet_state_dict
    from oracle.weights import model_config
    cfg = model_config('xs')
    ccfg = dict(cfg)
    ccfg.update(CN_DEFAULT)
    cn = DiTControlNet(device='cuda:0', **ccfg)
    cn.load_state_dict(make_controlnet_state_dict(cfg, CN_DEFAULT, 1))
    cond = t_((0.5 + 0.5 * uniform_pm1('tables.cond', 2 * 2 * 96, 3)).reshape(2, 1, 192).astype(np.float32))
    return cn, cond


def test_new_cn_scales_keep_the_graph_on_and_off_drop_it(lib, watch):
    m = get_model('xs', 1)
    cn, cond = _controlnet()
    try:
        w = watch(_prepare(TWO, controlnet=cn, condition=cond, conditioning_scale=0.8))
        w.check([('first run', None, True),
                 ('on', lambda: w.smp.set_cn_scales([0.5, 1.0]), True),
                 ('new values', lambda: w.smp.set_cn_scales([0.7, 0.2]), False),
                 ('off', lambda: w.smp.set_cn_scales(None), True)])
    finally:
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0


def test_new_pair_lengths_keep_the_graph_on_and_off_drop_it(lib, watch):
    m = get_model('xs', 1)
    cn, cond = _controlnet()
    cond4 = torch.cat([cond, cond], dim=0)   # (the CFG batch: both rows of a pair read the sample's condition)
    try:
        w = watch(_prepare(TWO, controlnet=cn, condition=cond, conditioning_scale=0.8))

        def pair(v):   # the pair's table, then the condition embed that is computed from it
            rc = lib.ezdit_sampler_set_pair_lengths(m._h, None if v is None else _arr(v), 0 if v is None else 2, w.st)
            cn.prepare_condition(cond4)
            return rc
        w.check([('first run', None, True),
                 ('on', lambda: pair([96, 80]), True),
                 ('new lengths', lambda: pair([70, 96]), False),
                 ('off', lambda: pair(None), True)])
    finally:   # (a detach takes the ControlNet's half of the table with it; the backbone's own goes here)
        assert lib.ezdit_sampler_attach_controlnet(m._h, None, 1.0) == 0
        m.set_lengths(None)


def test_a_rebind_ends_the_sampler_call(lib):
    """The same (B, L, Lc, slots) and buffer are bound again under a prepared call whose latents stay alive, and context and timesteps are prepared again: the
    run and the call-scoped setters must answer EZDIT_E_STATE "ezdit_sampler_begin first" -- not advance the old latents -- until the next prepare()."""
    from ezaudio_amd import _lib
    m = get_model('xs', 1)
    inp, meta = _case()
    ref = _finish(_prepare(TWO))
    smp = _prepare(TWO)
    st = C.c_void_p(smp.stream.cuda_stream)
    kept = smp.latents
    before = kept.clone()
    key = m._ws_key
    text, tm = t_(inp['ctx'][0:1]).repeat(2, 1, 1), t_(inp['ctx_mask'][0:1]).repeat(2, 1)
    un, um = t_(inp['ctx'][1:2]).repeat(2, 1, 1), t_(inp['ctx_mask'][1:2]).repeat(2, 1)
    with torch.cuda.stream(smp.stream):
        m._ws_key = None
        m.bind(*key)
        m.prepare_context(torch.cat([text, un], dim=0), torch.cat([tm, um], dim=0))
        m.prepare_timesteps([int(t) for t in _scheduler(K).timesteps], per_row=False)
        rc = lib.ezdit_sampler_run(m._h, 1, 1, st)
        assert rc == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error(), (rc, lib.ezdit_last_error())
        co = (_lib.EzditDdimCoef * (K * 2))(*[_lib.EzditDdimCoef(0.9, 0.4, 0.95, 0.3, 0.0) for _ in range(K * 2)])
        rc = lib.ezdit_sampler_set_sample_params(m._h, (C.c_float * 2)(3.0, 2.0), (C.c_float * 2)(0.0, 0.0), co, 2, st)
        assert rc == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error(), (rc, lib.ezdit_last_error())
        hist = torch.zeros_like(kept)
        for rc in (lib.ezdit_sampler_set_multistep(m._h, (C.c_float * K)(*([0.1] * K)), K, hist.data_ptr(), st),
                   lib.ezdit_sampler_set_start(m._h, _arr([0, 3]), 2, st),
                   lib.ezdit_sampler_set_canvas(m._h, _arr([0, 52]), 2, 148, 44, st)):
            assert rc == -3 and b'ezdit_sampler_begin' in lib.ezdit_last_error(), (rc, lib.ezdit_last_error())
    smp.stream.synchronize()
    assert torch.equal(kept, before), 'a refused call launches nothing'
    again = _finish(_prepare(TWO))
    assert torch.isfinite(again).all() and torch.equal(again, ref)
