"""The fp32 sums of the study kernels, pinned bit for bit (csrc/ica_reduce.h: the chain of a thread, the butterfly
of a wave, the order of a block's four waves, the lane-strided sum of an image's partials, and each study's number of
blocks per image).  The neighbouring tests hold these sums to 1e-5 of float64 and check batch invariance within one
build; an edit to a summation order passes both.  This one compares with tests/golden/study_sums.pt.

The fixture was recorded with the library of the commit before ica_reduce.h existed (ICA_HIP_LIB selects the
library the package loads), not with the code under test:

    ICA_HIP_LIB=<that commit's libica_hip.so> python -m tests.test_gpu_reduce_pinned [path]

It is one flat fp32 tensor: the outputs below in OUTPUTS order, shape after shape (the integer `changed` is at most
3 H W < 2^24, exact in fp32).  If these bits are ever changed on purpose, record it again in the same commit and say
so there.  floor_bits goes through logf and stays out; its own tests hold it.

Shapes (B, H, W), the smallest at which each piece can go wrong: (1, 8, 8) is one block and one partial;
(5, 192, 256) gives every study more than 64 partials per image, so the lane-strided loop wraps (noise and transfer
144 blocks, requant8 192, blur 3 x 24 tiles), has more images than the requant8 finish block has waves, and with
N = 5 noises on M = 2 targets leaves the 4-noise tile a remainder; (1, 512, 768) reaches every per-image block cap
(512 and 1024)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 8, 8), (5, 192, 256), (1, 512, 768)]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "study_sums.pt")
SIGMAS = [0.4, 1.0, 3.0]           # one blur_sweep chunk
OUTPUTS = ["noise_power", "noise_mse_in", "blur_mse", "sweep_mse", "pairs_mse_in", "score_clamp", "score_raw",
           "sse_orig", "sse_gen", "changed", "sqdiff_mean"]


def pairs_of(B):
    return B, min(B, 2)            # N noises x M targets


def sizes(shape):
    B = shape[0]
    N, M = pairs_of(B)
    return [B, B, B, B * len(SIGMAS), N * M, N * M, N * M, B, B, B, B]


def study_sums(shape):
    """name -> flat fp32 CPU tensor, from seeded CPU inputs."""
    from imagecompression_adversarial_amd import degrade, recompress, transfer
    from imagecompression_adversarial_amd import hip_ops as K
    B, H, W = shape
    N, M = pairs_of(B)
    g = torch.Generator().manual_seed(1000 * B + H + W)
    im = torch.rand((B, 3, H, W), generator=g).to(DEV)
    ref = torch.rand((B, 3, H, W), generator=g).to(DEV)
    noise = (torch.randn((B, 3, H, W), generator=g) * 0.2).to(DEV)            # clamps on both sides
    x_hat4 = (torch.rand((N * M, 1, H, W, 4), generator=g) * 2 - 0.5).to(DEV)
    x_s4 = (torch.rand((M, 1, H, W, 4), generator=g) * 2 - 0.5).to(DEV)
    out = {}
    _, out["noise_power"], out["noise_mse_in"] = degrade.apply_noise(im, noise)
    _, out["blur_mse"] = degrade.gaussian_blur(im, (5, 5), 0.8, clamp=True, ref=ref)
    _, out["sweep_mse"] = degrade.blur_sweep(im, SIGMAS, 1e-12)               # nothing fits: every candidate is scored
    _, out["pairs_mse_in"] = transfer.apply_pairs(im[:M].contiguous(), noise)
    out["score_clamp"] = transfer.score_pairs(x_hat4, x_s4, N, M, clamp=True)
    out["score_raw"] = transfer.score_pairs(x_hat4, x_s4, N, M, clamp=False)
    prev_q, _ = recompress.quant8_pack(ref)
    _, _, out["sse_orig"], out["sse_gen"], changed = recompress.requant8(x_hat4[:B].contiguous(), im, prev_q)
    assert int(changed.max()) < 1 << 24
    out["changed"] = changed.float()
    out["sqdiff_mean"] = K.sqdiff_mean(im, ref)
    out = {k: out[k].float().flatten().cpu() for k in OUTPUTS}
    assert [v.numel() for v in out.values()] == sizes(shape)
    assert all(bool(v.isfinite().all()) for v in out.values())
    return out


@pytest.fixture(scope="module")
def pinned():
    flat = torch.load(FIXTURE, map_location="cpu", weights_only=True)
    assert flat.dtype == torch.float32 and flat.numel() == sum(sum(sizes(s)) for s in SHAPES)
    per_shape = dict(zip(SHAPES, flat.split([sum(sizes(s)) for s in SHAPES])))
    return {s: dict(zip(OUTPUTS, per_shape[s].split(sizes(s)))) for s in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_study_sums_are_the_recorded_bits(pinned, shape):
    got = study_sums(shape)
    bad = [k for k in OUTPUTS if not torch.equal(got[k], pinned[shape][k])]
    for k in bad:
        print(shape, k, "got", got[k].tolist(), "recorded", pinned[shape][k].tolist())
    assert not bad


if __name__ == "__main__":
    import sys

    from imagecompression_adversarial_amd import _lib
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    print("recording", path, "with", _lib.LIB_PATH)
    torch.save(torch.cat([v for s in SHAPES for v in study_sums(s).values()]), path)
