"""CPU tests of the layer-wise error-propagation study: the restatement (tests/layer_compare_restatement.py) against the
reference's formulas written directly, its per-image semantics, the CLI's argparse errors, the e_ref tables behind
every bound of the GPU tests, and the condition on rounding ties.  No device."""
import pytest
import torch

from tests import layer_compare_restatement as S


@pytest.fixture(scope="module")
def cases():
    return {name: S.Case(name) for name in S.CASES}


@pytest.mark.parametrize("name", ["hyper-q1-1x64x128", "cheng2020-q1-1x64x64"])
def test_restatement_is_the_reference_formulas_at_batch_one(cases, name):
    """B = 1: the reference's whole-batch means are the per-image means, row by row and in the print order."""
    c = cases[name]
    enc, quant, dec, _, _ = S.study(c.P, c.im_adv, c.im_clean, c.model, torch.float64)
    r_enc, r_quant, r_dec = S.reference_formulas(c.P, c.im_adv, c.im_clean, c.model, torch.float64)
    assert len(r_enc) == 8 and len(r_dec) == (8 if c.model == "cheng2020" else 7)
    assert enc.shape == (1, 8) and dec.shape == (1, len(r_dec), 2) and quant.shape == (1, 2)
    assert torch.allclose(enc[0], torch.tensor(r_enc, dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.allclose(quant[0], torch.tensor(r_quant, dtype=torch.float64), rtol=1e-12, atol=0)
    assert torch.allclose(dec[0], torch.tensor(r_dec, dtype=torch.float64), rtol=1e-12, atol=0)
    # the first Quantization number reads the UNROUNDED adversarial latent: it differs from the second
    assert abs(r_quant[0] - r_quant[1]) > 1e-3 * r_quant[1]


def test_batch_rows_are_the_single_image_rows(cases):
    c = cases["hyper-q1-2x64x64"]
    enc, quant, dec, _, _ = S.study(c.P, c.im_adv, c.im_clean, c.model, torch.float64)
    for b in range(2):
        e1, q1, d1, _, _ = S.study(c.P, c.im_adv[b:b + 1], c.im_clean[b:b + 1], c.model, torch.float64)
        assert torch.allclose(enc[b], e1[0], rtol=1e-12, atol=0)
        assert torch.allclose(quant[b], q1[0], rtol=1e-12, atol=0)
        assert torch.allclose(dec[b], d1[0], rtol=1e-12, atol=0)
    assert not torch.allclose(enc[0], enc[1], rtol=1e-3)


def test_off_ties_moves_to_the_margin():
    y = torch.tensor([0.5, 0.52, 0.47, -1.5, -1.46, 2.0, 3.56, -0.449999])
    moved, share = S.off_ties(y)
    want = torch.tensor([0.55, 0.55, 0.45, -1.45, -1.45, 2.0, 3.56, -0.45])
    assert torch.allclose(moved, want, atol=1e-6)
    assert share == pytest.approx(5 / 8)        # the fp32 -0.449999 lies 0.050001 from -0.5: it stays
    assert torch.equal(torch.round(moved.double()), torch.round(moved))


def test_tie_share_below_the_cap(cases):
    """The latents the quant / decoder rows are tested from: fewer than 12 % of the elements had to move, and none
    is left within the margin of a half-integer (so the fp32 and float64 roundings agree)."""
    for name, c in cases.items():
        print(f"{name}: moved shares {c.shares()}, spread gain {c.gain}")
        assert all(v < S.TIE_SHARE_CAP for v in c.shares().values())
        assert 3.0 <= float(c.y_clean_s.std()) < 6.5 and float(c.y_clean_s.abs().max()) > 8
        for y in (c.y_adv, c.y_clean, c.y_adv_s, c.y_clean_s):
            d = (y.double() - (torch.floor(y.double()) + 0.5)).abs()
            assert float(d.min()) > S.TIE_MARGIN - 1e-5


def test_e_ref_table_of_the_study(cases):
    """Prints e_ref (fp32 CPU restatement against float64, relative per row, the largest of the side) and holds the
    fp32 restatement to each committed bound; a bound is 4 max(e_ref, 2^-24) rounded up to one digit."""
    smallest = min(c.smallest_mse() for c in cases.values())
    print(f"smallest mse of any row: {smallest:.3e}")
    assert smallest > 1e-7          # far above the rounding of O(1) activations squared (2^-48)
    assert S.SMALLEST_MSE == pytest.approx(smallest, rel=0.05)
    for name, c in cases.items():
        e = c.e_ref()
        print(f'    "{name}": dict(' + ", ".join(f"{k}={S.bound_of(v):g}" for k, v in e.items()) + "),")
        print("    # e_ref " + ", ".join(f"{v:.2e}" for v in e.values()))
        for k, v in e.items():
            assert v <= S.STUDY_TOL[name][k], (name, k, v)


def test_e_ref_table_of_the_kernel():
    for shape in S.KERNEL_SHAPES:
        e = S.kernel_e_ref(shape)
        key = S.shape_key(shape)
        print(f'    "{key}": dict(' + ", ".join(f"{k}={S.bound_of(v):g}" for k, v in e.items()) + "),")
        print("    # e_ref " + ", ".join(f"{v:.2e}" for v in e.values()))
        for k, v in e.items():
            assert v <= S.KERNEL_TOL[key][k], (key, k, v)


def test_kernel_case_ties_are_ties():
    a, b, _ = S.kernel_case((2, 128, 32, 48))
    n = len(S.TIES)
    ties = torch.tensor(S.TIES)
    assert torch.equal(a.reshape(2, -1)[:, :n], ties.expand(2, n))
    frac = (ties.double() - torch.floor(ties.double()))
    assert int((frac == 0.5).sum()) >= 9                     # exact ties, the large ones included
    assert float(torch.round(torch.tensor(2.5))) == 2.0 and float(torch.round(torch.tensor(-0.5))) == 0.0
    r = S.kernel_ref(a, b, a)
    assert float(r["quant1"].min()) >= 4.0                   # small integers: a tie rule off by one shows


# --------------------------------------------------------------------------- #
# the CLI's argument errors (no model is built)
# --------------------------------------------------------------------------- #
BASE = ["-s", "synthetic:1x64x64", "--synthetic-weights", "-q", "1"]


@pytest.mark.parametrize("extra", [[], ["--attack", "--gauss", "0.01"], ["-t", "x*.png", "--attack"],
                                   ["-t", "x*.png", "--gauss", "0.01"], ["-t", "x*.png", "--attack", "--gauss", "0.1"],
                                   ["--gauss", "-1"], ["--gauss", "nan"]])
def test_cli_needs_exactly_one_source_of_adversarial_images(extra, monkeypatch):
    from imagecompression_adversarial_amd import layer_compare
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        layer_compare.parse(BASE + extra)
    assert e.value.code == 2


def test_cli_refuses_a_torchrun_launch(monkeypatch):
    from imagecompression_adversarial_amd import layer_compare
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        layer_compare.parse(BASE + ["--gauss", "0.01"])
    assert e.value.code == 2
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert layer_compare.parse(BASE + ["--gauss", "0.01"]).gauss == 0.01


def test_cli_refuses_the_debug_model(monkeypatch):
    from imagecompression_adversarial_amd import layer_compare
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(NotImplementedError, match="two"):
        layer_compare.main(BASE + ["--gauss", "0.01", "-m", "debug"])


def test_gauss_noise_is_per_image_and_seeded():
    from imagecompression_adversarial_amd import layer_compare
    im = torch.rand((3, 3, 8, 8), generator=torch.Generator().manual_seed(5))
    adv = layer_compare.gauss_adv(im, 0.01)
    assert torch.equal(adv[1:2], layer_compare.gauss_adv(im[1:2], 0.01, first_index=1))
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
    assert torch.equal(layer_compare.gauss_adv(im, 0.0), im)
    assert 0.005 < float((adv - im).std()) < 0.012
