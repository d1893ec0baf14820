"""CPU tests of the groundwork for adaptive projected guidance (tests/apg_emul.py): the definition in float64 and its identities, an fp32 emulation of the
order of operations a two-pass row kernel would use (64 chunked partial sums in fp32, the final reduction in double) and its distance from float64 -- the floor
a GPU gate can be built on -- nine deliberate mistakes that must each stand well clear of that floor, and the oracle-loop goldens of tools/mint_apg_golden.py.
The kernels, the C ABI and the `apg` argument themselves are not part of the tree yet."""
import numpy as np

from tests import apg_emul as E
from tests.util import DIFF, load_golden


def mid_schedule_coef():
    """(sa, sb, c_x0, c_dir, sigma) of step 7 of 50, eta 0: a step at which x0c is not a multiple of c (at step 0, t = 999, sa = 0 and x0c = -c)."""
    from ezaudio_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(**DIFF)
    sch.set_timesteps(50)
    co = sch._coef(int(sch.timesteps[7]), 0.0)
    assert 0.05 < co[0] < 0.95 and co[4] == 0.0
    return co


# ---------------------------------------------------------------------------------------------------
# 1. the definition: identities in float64
# ---------------------------------------------------------------------------------------------------
def _vectors(seed=3, n=(16, 37)):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(n) * 1.3
    u = 0.6 * c + 0.8 * rng.standard_normal(n)
    return c, u, rng.standard_normal(n), 0.5 * rng.standard_normal(n)


def test_eta_1_without_cap_and_momentum_is_plain_cfg():
    from oracle.sampler import cfg_combine
    sa, sb, cx0, cdir, _ = mid_schedule_coef()
    c, u, x, m = _vectors()
    for w in (1.0, 2.0, 7.5):
        x0, v, d, (nd, s, a) = E.apg_fp64(c, u, x, None, sa, sb, w, 1.0, 0.0, 0.0)
        vc = cfg_combine(c, u, w)                                      # oracle/sampler.py, pushed through the DDIM expression
        want = cx0 * (sa * x - sb * vc) + cdir * (sa * vc + sb * x)
        got = cx0 * x0 + cdir * (sa * v + sb * x)
        assert s == 1.0 and E.rel_l2(got, want) < 1e-13, w
        assert E.rel_l2(x0, sa * x - sb * v) < 1e-13                   # x0 and v describe one prediction


def test_eta_0_leaves_nothing_parallel_to_x0c_and_the_cap_holds():
    sa, sb, _, _, _ = mid_schedule_coef()
    c, u, x, m = _vectors(5)
    x0c = sa * x - sb * c
    for beta, r in ((0.0, 0.0), (-0.5, 0.0), (-0.5, 3.0), (0.3, 1e-3)):
        x0, v, d, (nd, s, a) = E.apg_fp64(c, u, x, m, sa, sb, 4.0, 0.0, r, beta)
        U = (x0 - x0c) / 3.0
        assert abs((U * x0c).sum()) <= 1e-12 * np.linalg.norm(U) * np.linalg.norm(x0c), (beta, r)
        if r > 0:
            assert nd > r and s < 1.0                                  # the cap bites on these inputs ...
            assert np.linalg.norm(s * d) <= r * (1 + 1e-12)            # ... and holds
        assert E.rel_l2(d, sb * (u - c) + beta * m) < 1e-13            # the momentum is stored before the cap
    # eta_apg keeps that share of the parallel part
    x0h, _, d, (_, s, a) = E.apg_fp64(c, u, x, m, sa, sb, 4.0, 0.25, 0.0, 0.0)
    par = (d * x0c).sum() / (x0c * x0c).sum() * x0c
    assert E.rel_l2((x0h - x0c) / 3.0, (d - par) + 0.25 * par) < 1e-12
    # a prediction of all zeros has no direction to project on: a = 0, U = s d
    z = np.zeros_like(c)
    x0, _, d, (_, _, a) = E.apg_fp64(z, u, z, None, sa, sb, 4.0, 0.0, 0.0, 0.0)
    assert a == 0.0 and np.array_equal(x0, 3.0 * d)


# ---------------------------------------------------------------------------------------------------
# 2. the emulation's floor and the nine mistakes
# ---------------------------------------------------------------------------------------------------
def test_every_deliberate_mistake_stands_ten_floors_clear_of_float64():
    """The inputs are apg_emul.operator_case's at L = 150, step 7 of 50, the cap at half the measured |d|, with lengths [131, 77, 1]: the sample whose sums
    matter (sample 0: cap and projection) has padded frames, so norms taken over them show.  The floor is the larger of the emulation's distances on these
    inputs and on the operator's three cases.  Measured: floor 8.2e-8, the nearest mistakes 'project_on_c' (2.6e-2) and 'norm_over_padding' (5.4e-2)."""
    co = mid_schedule_coef()
    case = E.operator_case(150, [131, 77, 1], co)
    pred, lat, hist, mom, params, ln = case
    nd = E.apg_fp64(pred[0, :, :131], pred[3, :, :131], lat[0, :, :131], mom[0, :, :131], float(params[0, 2]), float(params[0, 3]), 5.0, 0.0, 0.0, -0.5)[3][0]
    assert 0 < params[0, 9] < nd                                       # the cap lies below the measured |d|: it bites
    floor, far = E.floor_and_mistakes(case)
    for L, lens in ((96, None), (150, None), (150, [150, 77, 1])):
        floor = max(floor, E.floor_and_mistakes(E.operator_case(L, lens, co))[0])
    print(f'APG emulation floor (largest rel-L2 vs fp64 over latents, x0_hist, momentum): {floor:.3e}')
    for mk in E.MISTAKES:
        print(f'  mistake {mk:20s}: {far[mk]:.3e} = {far[mk] / floor:.1f} floors')
    assert 0 < floor < 1e-6
    assert set(far) == set(E.MISTAKES) and len(E.MISTAKES) == 9
    for mk, dist in far.items():
        assert dist >= 10 * floor, (mk, dist, floor)
    # the emulation without a mistake is the definition: every output, every sample, padded frames exactly zero
    got = E.step_emul(pred, lat, hist, mom, params, ln)
    for t in got[:2]:
        for p, n in enumerate(ln):
            assert not t[p, :, n:].any()
    assert np.array_equal(got[2][2], mom[2])                           # a sample without guidance keeps its momentum rows


# ---------------------------------------------------------------------------------------------------
# 3. the goldens of the fused loop (tools/mint_apg_golden.py)
# ---------------------------------------------------------------------------------------------------
def test_the_loop_goldens_tell_apg_from_plain_cfg():
    """tests/golden/sampler_apg_xs.npz: the numpy oracle's 20-step loop on smp_xs_e0's inputs with the APG update in float64, DDIM and dpmpp_2m.  The mint tool
    chose the cap from |d| of step 0 so that each golden lies at least 10 loop gates (10 x 2e-2) from the plain-CFG loop of the same inputs."""
    g, meta = load_golden('sampler_apg_xs')
    assert meta['base'] == 'smp_xs_e0' and meta['steps'] == 20 and meta['guidance_rescale'] == 0.0
    assert (meta['eta_apg'], meta['momentum']) == (0.0, -0.5) and 0 < meta['norm_threshold'] < meta['d0']
    for key, dist in (('latent_ddim', meta['dist_ddim']), ('latent_2m', meta['dist_2m'])):
        assert g[key].shape == (1, 128, meta['L']) and np.isfinite(g[key]).all()
        assert dist >= 10 * 2e-2, (key, dist)
    assert E.rel_l2(g['latent_2m'], g['latent_ddim']) > 1e-3          # two solvers, two goldens
