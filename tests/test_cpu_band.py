"""CPU side of the band study and the band-limited attack (DESIGN.md "Band VI"): the properties of the float64
restatement the GPU tests compare with, that its guards were measured, the input precondition of the gradient cases,
and the parsing and refusals of band_vi / attack_band, which happen before the device library is touched."""
import pytest
import torch

from tests import band_restatement as P


def _x(shape=(2, 16, 24), seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((shape[0], 3, shape[1], shape[2]), generator=g, dtype=torch.float64)


def test_dct_matrix_is_orthonormal():
    D = P.dct_matrix()
    assert float((D @ D.T - torch.eye(8, dtype=torch.float64)).abs().max()) < 1e-15
    tab = P.band_table()
    assert [int((tab == k).sum()) for k in range(8)] == [2 * k + 1 for k in range(8)]


@pytest.mark.parametrize("mask", [0b1, 0b00000111, 0b10100110, 0xFE, 0xFF, 0])
def test_projection_is_idempotent_and_symmetric(mask):
    a, b = _x(seed=1), _x(seed=2)
    pa = P.project(a, mask)
    assert float((P.project(pa, mask) - pa).abs().max()) < 1e-14
    assert abs(float((pa * b).sum() - (a * P.project(b, mask)).sum())) < 1e-11
    if mask == 0:
        assert float(pa.abs().max()) == 0.0


def test_bands_sum_to_identity_and_parseval():
    x = _x((3, 24, 40), 3)
    assert float((sum(P.project(x, 1 << k) for k in range(8)) - x).abs().max()) < 1e-14
    assert float((P.project(x, P.preset_masks("lowpass")[7]) - x).abs().max()) < 1e-14
    e = P.energies(x)
    assert float((e.sum(1) - (x ** 2).mean(dim=(1, 2, 3))).abs().max()) < 1e-14
    for k in range(8):      # the energy of band k is that of its projection
        assert float((e[:, k] - (P.project(x, 1 << k) ** 2).mean(dim=(1, 2, 3))).abs().max()) < 1e-14


@pytest.mark.parametrize("name", list(P.GRAD_CASES))
def test_autograd_equals_closed_form(name):
    noise, im_s, g_net, mask, thr = P.grad_case(name)
    im_in, loss_i, cheap, g = P.step(noise, im_s, g_net, mask, thr)
    want = P.step_closed_form(noise, im_s, g_net, mask, thr)
    assert cheap.tolist() == [True, False]
    assert all(v > 2 * thr or v < thr / 2 for v in loss_i.tolist())
    assert float(want.abs().max()) > 0 and float((g - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("name", list(P.GRAD_CASES))
def test_gradient_case_precondition(name):
    """No element of the float64 u = im_s + P_S(nc) lies within U_MARGIN of 0 or 1 (cap on left-out elements: zero),
    both clamps and both noise bounds act somewhere, and the compares of the noise with +-eps are those of the fp32
    values cast up."""
    noise, im_s, g_net, mask, thr = P.grad_case(name)
    _, u, _, _ = P.forward(noise.double(), im_s.double(), mask)
    assert float(torch.minimum(u.abs(), (u - 1).abs()).min()) > P.U_MARGIN
    assert int((u < 0).sum()) > 0 and int((u > 1).sum()) > 0
    e = float(torch.tensor(P.EPS, dtype=torch.float32))
    assert int((noise > e).sum()) > 0 and int((noise < -e).sum()) > 0
    assert torch.equal(noise.double() > e, noise > torch.tensor(P.EPS)) and int((noise.abs() == e).sum()) == 0


@pytest.mark.parametrize("what", ["PROJ", "ENERGY", "GRAD"])
def test_guards_are_four_times_the_measured_twin(what):
    fresh = {"PROJ": P.measure_proj, "ENERGY": P.measure_energy, "GRAD": P.measure_grad}[what]()
    guard, recorded = getattr(P, "GUARD_" + what), getattr(P, "MEASURED_" + what)
    print(what, "fresh", fresh, "recorded", recorded, "guard", guard)
    assert guard == 4 * recorded
    assert 0.5 <= guard / (4 * fresh) <= 2.0


def test_presets_and_parsing():
    from imagecompression_adversarial_amd import band_vi as BV
    assert BV.preset_masks("only") == [1, 2, 4, 8, 16, 32, 64, 128]
    assert BV.preset_masks("lowpass") == [1, 3, 7, 15, 31, 63, 127, 255]
    assert BV.preset_masks("without") == [254, 253, 251, 247, 239, 223, 191, 127]
    for name in P.PRESETS:
        assert BV.preset_masks(name) == P.preset_masks(name)
    assert torch.equal(BV.band_index(), P.band_table())
    assert BV.parse_bands("0-2,5") == 0b100111
    assert BV.parse_bands("7") == 128 and BV.parse_bands(" 3 , 0-1 ") == 0b1011 and BV.parse_bands("0-7") == 255
    assert BV.parse_bands(6) == 6 and BV.mask_label(0b100111) == "0,1,2,5"
    for bad in ("", "8", "2-1", "a", "1-2-3", "0,,1", "-1", None, 256, -1, True, 1.5):
        with pytest.raises(ValueError):
            BV.parse_bands(bad)
    with pytest.raises(ValueError):
        BV.preset_masks("highpass")


def _no_device(monkeypatch):
    from imagecompression_adversarial_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "lib", boom)


REFUSED = [dict(rate=True), dict(target="t.png"), dict(roi=[0, 8, 0, 8]), dict(coupled=True), dict(pad=8),
           dict(defend=True), dict(model="debug"), dict(att_metric="ms-ssim")]


@pytest.mark.parametrize("kw", REFUSED, ids=[next(iter(k)) for k in REFUSED])
def test_band_guard_refuses(monkeypatch, kw):
    from imagecompression_adversarial_amd import band_vi as BV
    _no_device(monkeypatch)
    BV.band_guard(model="hyper")
    with pytest.raises(NotImplementedError):
        BV.band_guard(**kw)


@pytest.mark.parametrize("flags", [["-r"], ["--mask_loc", "0", "8", "0", "8"], ["-p", "8"], ["--defend"],
                                   ["-m", "debug"], ["-att_metric", "ms-ssim"]], ids=lambda f: f[0])
def test_cli_refuses_before_the_device(monkeypatch, flags):
    from imagecompression_adversarial_amd import attack_band
    _no_device(monkeypatch)
    argv = ["-q", "1", "-metric", "mse", "-s", "none*.png", "--attack", "--bands", "0-2", "--synthetic-weights"]
    with pytest.raises(NotImplementedError):
        attack_band.main(argv + flags)


def test_cli_argument_errors(monkeypatch):
    from imagecompression_adversarial_amd import attack_band
    _no_device(monkeypatch)
    for argv in (["-s", "a.png"], ["-s", "a.png", "-t", "b.png", "--attack"],
                 ["-s", "a.png", "-t", "b.png", "--bands", "0-2"], ["-s", "a.png", "--attack", "--bands", "9"],
                 ["-s", "a.png", "--attack", "--preset", "highpass"]):
        with pytest.raises(SystemExit):
            attack_band.main(argv)


def test_shapes_that_are_no_multiple_of_8_raise(monkeypatch):
    from imagecompression_adversarial_amd import band_vi as BV
    _no_device(monkeypatch)
    for shape in ((1, 3, 12, 16), (1, 3, 16, 20), (1, 3, 4, 8)):
        x = torch.zeros(shape)
        with pytest.raises(ValueError):
            BV.project(x, 1)
        with pytest.raises(ValueError):
            BV.split_bands(x, x, "only")
        with pytest.raises(ValueError):
            BV.BandAttackLoop(None, x, "0-2")
    with pytest.raises(ValueError):
        BV.split_bands(torch.zeros((1, 3, 8, 8)), torch.zeros((2, 3, 8, 8)), "only")
    with pytest.raises(ValueError):
        BV.project(torch.zeros((1, 3, 8, 8)), 256)
