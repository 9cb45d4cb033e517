"""CPU tests of the re-compression study: the restatement tests/recompress_restatement.py against a real PNG round
trip, the arithmetic facts ica_recompress.hip relies on, and what recompress / the recompression CLI refuse before
anything is launched."""
import numpy as np
import pytest
import torch

from tests import recompress_restatement as R


def test_restatement_roundtrip_equals_png_roundtrip_on_random_data():
    x = R.rand_image((2, 3, 64, 128), 1)
    u8, im = R.roundtrip(x)
    u8p, imp = R.roundtrip_png(x)
    assert u8.dtype == np.uint8 and np.array_equal(u8, u8p) and torch.equal(im, imp)
    assert im.dtype == torch.float32 and len(np.unique(u8)) == 256


def test_roundtrip_of_every_code_is_the_identity():
    codes = (torch.arange(256).double() / 255.0).float().view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    u8, im = R.roundtrip(codes)
    u8p, imp = R.roundtrip_png(codes)
    assert np.array_equal(u8[0, :, :, 0].reshape(-1), np.arange(256, dtype=np.uint8))
    assert np.array_equal(u8, u8p) and torch.equal(im, codes) and torch.equal(imp, codes)
    assert torch.equal(R.decode(R.pack(u8)), codes) and torch.equal(R.unpack(R.pack(u8))[0, 1], R.unpack(R.pack(u8))[0, 0])


def test_exact_halfway_products_round_to_even():
    ties = R.exact_halfway_values()
    assert len(ties) >= 32
    x = torch.tensor(ties, dtype=torch.float32)
    prod = x.numpy() * np.float32(255.0)
    assert prod.dtype == np.float32 and np.array_equal(prod - np.floor(prod), np.full(len(ties), 0.5, np.float32))
    n = len(ties)
    img = torch.zeros((1, 3, 1, n))
    img[0, :, 0] = x
    u8, _ = R.roundtrip(img)
    u8p, _ = R.roundtrip_png(img)
    got = u8[0, 0, :, 0].astype(np.int64)
    assert np.array_equal(u8, u8p) and np.all(got % 2 == 0) and np.all(np.abs(got - prod) == 0.5)
    assert torch.equal(torch.from_numpy(got), torch.round(torch.from_numpy(prod)).long())      # torch rounds alike


def test_out_of_range_input_is_clamped_first():
    x = torch.tensor([-0.5, -1e-9, -0.0, 0.0, 0.0019, 0.002, 0.998, 0.9981, 1.0, 1.0 + 1e-6, 1.5, 300.0])
    img = x.view(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    u8, im = R.roundtrip(img)
    u8p, imp = R.roundtrip_png(img)
    assert np.array_equal(u8, u8p) and torch.equal(im, imp)
    assert u8[0, 0, :, 0].tolist() == [0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 255, 255]
    nan = torch.full((1, 3, 1, 4), float("nan"))
    assert not R.roundtrip(nan)[0].any()                              # the documented NaN code


def test_float32_quotient_equals_the_float64_read_for_every_code():
    k = np.arange(256)
    f32 = k.astype(np.float32) / np.float32(255.0)
    assert f32.dtype == np.float32
    assert np.array_equal(f32, (k.astype(np.float64) / 255.0).astype(np.float32))
    assert np.array_equal(np.round(f32 * np.float32(255.0)), k.astype(np.float32))
    recip = k.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip != f32).sum()) > 0                              # why the kernel divides


def test_requant_restatement_counts_and_sums():
    x, orig, prev, m = R.kernel_case(2, 64, 64, 3)
    assert m >= 32
    r = R.requant(x, orig, prev)
    assert r["q"].dtype == torch.int32 and int(r["q"].max()) < 1 << 24
    assert torch.equal(R.decode(r["q"]), r["next"])
    assert all(0 < int(c) < 3 * 64 * 64 for c in r["changed"])
    same = R.requant(x, orig, r["q"])
    assert not same["changed"].any() and not same["sse_gen"].any() and torch.equal(same["q"], r["q"])


def test_validation_raises_before_the_library_is_loaded():
    from imagecompression_adversarial_amd import _lib, recompress
    loaded = _lib._lib
    ok = torch.zeros((1, 3, 64, 64))
    cases = [
        (torch.zeros((3, 64, 64)), 1, 8, "not a \\[B, 3, H, W\\] batch"),
        (torch.zeros((1, 1, 64, 64)), 1, 8, "not a \\[B, 3, H, W\\] batch"),
        (torch.zeros((0, 3, 64, 64)), 1, 8, "not a \\[B, 3, H, W\\] batch"),
        (ok.double(), 1, 8, "float32"),
        (torch.zeros((1, 3, 64, 128))[:, :, :, ::2], 1, 8, "contiguous"),
        (torch.zeros((1, 3, 64, 96)), 1, 8, "multiples of 64"),
        (torch.zeros((1, 3, 32, 64)), 1, 8, "multiples of 64"),
        (ok, 0, 8, "generations"),
        (ok, 2.0, 8, "generations"),
        (ok, 1, 0, "check_every"),
        (ok, 1, 8, "device tensor"),
    ]
    for im, gens, every, msg in cases:
        with pytest.raises(ValueError, match=msg):
            recompress.validate(im, gens, every)
    with pytest.raises(ValueError, match="device tensor"):
        recompress.recompress(None, ok, 3)
    with pytest.raises(ValueError, match="multiples of 64"):
        recompress.rd_metrics(None, torch.zeros((1, 3, 64, 100)))
    assert _lib._lib is loaded


def test_cli_refuses_other_defences_and_an_empty_glob(tmp_path):
    from imagecompression_adversarial_amd import recompression
    base = ["-m", "hyper", "-q", "1", "--synthetic-weights", "-steps", "2"]
    with pytest.raises(ValueError, match="always 'ensemble'"):
        recompression.main(base + ["-s", "synthetic:1x64x64", "--defend", "--defend_m", "resize"])
    with pytest.raises(ValueError, match="no image matches"):
        recompression.main(base + ["-s", str(tmp_path / "nothing*.png")])
    with pytest.raises(ValueError, match="at least one generation"):
        recompression.main(["-s", "synthetic:1x64x64", "-steps", "0"])
