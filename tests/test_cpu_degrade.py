"""CPU tests of the degradation baselines: the restatement tests/degrade_restatement.py against scipy, the host
pieces of imagecompression_adversarial_amd.degrade and the random_noise CLI's argument handling, and the margins of
the inputs tests/test_gpu_degrade.py pins for the sigma search."""
import math

import numpy as np
import pytest
import torch

from tests import degrade_restatement as R


@pytest.fixture(scope="module")
def DG():
    from imagecompression_adversarial_amd import degrade
    return degrade


@pytest.fixture(scope="module")
def RN():
    from imagecompression_adversarial_amd import random_noise
    return random_noise


# --------------------------------------------------------------------------- #
# the restatement itself
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("ksize,sigma", [((5, 9), 0.5), ((5, 5), 1.0), ((5, 5), 5.0)])
def test_restatement_matches_scipy_in_float64(ksize, sigma):
    from scipy import ndimage
    kx, ky = ksize
    x = R.rand_image((2, 3, 12, 20), 1).double()
    got = R.blur(x, ksize, sigma, torch.float64, torch.float64)
    k2 = R.kernel2d(R.taps(kx, sigma, torch.float64), R.taps(ky, sigma, torch.float64)).numpy()
    for b in range(2):
        for c in range(3):
            ref = ndimage.correlate(x[b, c].numpy(), k2, mode="mirror")
            assert np.abs(got[b, c].numpy() - ref).max() < 1e-15
    # fp32 run of the same restatement against float64 (the issue measured 2.9e-7 at (5, 9), sigma 0.5)
    got32 = R.blur(x.float(), ksize, sigma, torch.float32, torch.float32)
    assert float((got32.double() - got).abs().max()) < (kx * ky + 4) * R.EPS24


def test_gaussian_taps_bit_equal_and_normalised(DG):
    for k in (1, 3, 5, 7, 9):
        for sigma in (0.005, 0.3, 0.5, 1.0, 1.06, 5.0):
            t = DG.gaussian_taps(k, sigma)
            assert t.dtype == torch.float32 and torch.equal(t, R.taps(k, sigma))
            assert abs(float(t.double().sum()) - 1) < 4 * R.EPS24
    ident = torch.zeros(5)
    ident[2] = 1
    assert torch.equal(DG.gaussian_taps(5, 0.005), ident)       # the last candidate is the identity kernel
    assert torch.equal(DG.gaussian_taps(1, 0.7), torch.ones(1))


def test_schedule_is_the_python_loop(DG):
    s = DG.sigma_schedule()
    assert len(s) == 1000 and s[0] == 5.0
    sigma, loop = 5.0, [5.0]
    for _ in range(999):
        sigma = sigma - 0.005
        loop.append(sigma)
    assert s == loop                      # bit-equal doubles
    assert s == R.schedule()
    assert s[-1] > 0.0025 and s[-1] - 0.005 <= 0.0025
    assert len(DG.sigma_schedule(5.0, 0.6)) == 8


def test_validate_errors(DG):
    DG.validate(64, 64, (5, 9), 0.5)
    DG.validate(8, 8, (9, 9), [0.3, 5.0])
    DG.validate(5, 4, (1, 9), 0.5, noise=1e-4)
    bad = [dict(kernel_size=(4, 5)), dict(kernel_size=(5, 11)), dict(kernel_size=(0, 5)), dict(kernel_size=5),
           dict(kernel_size=(5.0, 5)), dict(kernel_size=(5, 5, 5)), dict(sigma=0.0), dict(sigma=-1.0),
           dict(sigma=float("nan")), dict(sigma=[0.5, "a"]), dict(noise=0.0), dict(noise=-1e-4),
           dict(noise=float("inf")), dict(noise=1e-4, factor=0.0), dict(noise=1e-4, step=0.0),
           dict(noise=1e-4, start=0.001, step=0.005), dict(noise=1e-4, start=5.0, step=1e-7)]
    for kw in bad:
        with pytest.raises(ValueError):
            DG.validate(64, 64, **kw)
    for H, W, ks in [(64, 66, (5, 5)), (4, 64, (5, 9)), (64, 4, (9, 5)), (0, 64, (5, 5)), (64.0, 64, (5, 5))]:
        with pytest.raises(ValueError):
            DG.validate(H, W, ks)
    # bad tensors are refused before any launch (no device is touched)
    with pytest.raises(ValueError):
        DG.gaussian_blur(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError):
        DG.apply_noise(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(RuntimeError):
        DG.gaussian_blur(torch.zeros(1, 3, 8, 8))          # a CPU tensor: there is no CPU path


# --------------------------------------------------------------------------- #
# CLI argument handling
# --------------------------------------------------------------------------- #
def test_cli_modes_and_plans(RN):
    parse = RN.config().parse_args
    a = parse(["-s", "None", "-t", "k*.png", "-noise", "1e-3"])
    assert RN.mode(a) == "generate" and RN.sweep_plan(a) == [] and a.blur_dir == "./attack/kodak/blur"
    assert RN.blur_file_name("/data/kodak/kodim07.png") == "./attack/kodak/blur/kodim07.png"
    assert RN.blur_file_name("a/b.c.png", "out/") == "out/b.png"
    with pytest.raises(ValueError):
        RN.mode(parse(["-s", "None"]))

    a = parse(["-degrade", "deblur", "-s", "blur/*.png", "-t", "k*.png", "-q", "2"])
    assert RN.mode(a) == "deblur" and RN.sweep_plan(a) == [(2, None)]
    a = parse(["-degrade", "deblur", "-s", "blur/*.png", "-t", "k*.png", "-q", "0", "-m", "cheng2020"])
    assert RN.sweep_plan(a) == [(q, None) for q in range(1, 7)]
    with pytest.raises(ValueError):
        RN.mode(parse(["-degrade", "deblur", "-s", "blur/*.png"]))
    with pytest.raises(ValueError):
        RN.mode(parse(["-degrade", "denoise", "-s", "x.png"]))

    a = parse(["-s", "k*.png", "-q", "3", "-noise", "1e-3"])
    assert RN.mode(a) == "noise" and RN.sweep_plan(a) == [(3, 1e-3)]
    a = parse(["-s", "k*.png", "-q", "0"])
    plan = RN.sweep_plan(a)
    assert len(plan) == 32 and plan[0] == (1, 1e-5) and plan[-1] == (8, 1e-2)
    assert [n for q, n in plan if q == 4] == [1e-5, 1e-4, 1e-3, 1e-2]


def test_noise_stream_is_the_reference_stream():
    """The CLI samples per image, in order, after manual_seed(0): the same values as the reference's m.sample."""
    torch.manual_seed(0)
    m = torch.distributions.normal.Normal(0.0, 1e-4 ** 0.5)
    a, b = m.sample((1, 3, 64, 64)), m.sample((1, 3, 64, 128))
    torch.manual_seed(0)
    a2 = torch.randn((1, 3, 64, 64)) * (1e-4 ** 0.5)
    assert torch.allclose(a, a2, rtol=1e-6, atol=0) and not torch.equal(a[0, 0, 0, :8], b[0, 0, 0, :8])


# --------------------------------------------------------------------------- #
# the search: why a linear scan, and the margins of the pinned GPU inputs
# --------------------------------------------------------------------------- #
def test_checkerboard_mse_is_not_monotone_in_sigma():
    x, noise, ksize, _, _, sig, mse = R.search_case("checkerboard")
    T = 1.01 * noise
    row = mse[0].tolist()
    assert math.isclose(row[0], 9.799e-5, rel_tol=1e-3) and row[0] < T * 0.98         # fits at once: k = 0
    assert math.isclose(row[500], 1.0087e-4, rel_tol=1e-3)
    assert math.isclose(max(row), 1.0491e-4, rel_tol=1e-3) and max(row) > T
    assert R.scan(mse[0], T) == 0
    last_false = max(j for j, v in enumerate(row) if v > T)
    assert last_false + 1 == 853                                # where a first-true-after-last-false search lands
    # the side tap of the normalised 5-tap Gaussian is itself not monotone in sigma
    side = [float(R.taps(5, s, torch.float64)[1]) for s in (5.0, 1.06, 0.5)]
    assert side[1] > side[0] and side[1] > side[2]
    d2 = 1.05e-4
    assert math.isclose(row[0] / d2, 0.934, abs_tol=2e-3) and math.isclose(max(row) / d2, 0.999, abs_tol=2e-3)


@pytest.mark.parametrize("name", list(R.SEARCH_CASES))
def test_pinned_search_inputs_have_margin(name):
    x, noise, ksize, start, step, sig, mse = R.search_case(name)
    T = 1.01 * noise
    delta = R.search_delta(ksize, T)
    if noise == 1e-4:
        assert math.isclose(delta, 3.6e-4, rel_tol=0.05)
    for b in range(x.shape[0]):
        assert R.has_margin(mse[b], T, delta), (name, b)
        ok, early = R.check_index(mse[b], R.scan(mse[b], T), T, delta)
        assert ok and not early


def test_pinned_search_inputs_cover_the_cases():
    ks = {n: [R.scan(row, 1.01 * R.search_case(n)[1]) for row in R.search_case(n)[6]] for n in R.SEARCH_CASES}
    assert ks["smooth_1e-4"] == [902, 900]
    assert all(800 < k < 900 for k in ks["smooth_1e-3"])
    mixed = ks["mixed"]
    assert 0 in mixed and len({k // 32 for k in mixed}) >= 3          # k = 0 and three different chunks
    assert ks["never"] == [-1, 0] and len(R.search_case("never")[5]) == 8
    assert ks["checkerboard"] == [0]
