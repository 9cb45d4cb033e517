"""CPU tests of the perturbation-transfer study: the restatement tests/transfer_restatement.py against a hand-computed
case, and the host pieces of imagecompression_adversarial_amd.transfer and the transfer_noise CLI (chunking, the NaN
rules, the parser, argument checks before any launch)."""
import math

import pytest
import torch

from tests import transfer_restatement as R


@pytest.fixture(scope="module")
def T():
    from imagecompression_adversarial_amd import transfer
    return transfer


@pytest.fixture(scope="module")
def TN():
    from imagecompression_adversarial_amd import transfer_noise
    return transfer_noise


def const(values, hw=(2, 4)):
    return torch.stack([torch.full((3,) + hw, v) for v in values])


# --------------------------------------------------------------------------- #
# the restatement itself
# --------------------------------------------------------------------------- #
def test_restatement_hand_computed_2x2():
    """Constant images make every mean a single squared difference.
    im = (0.5, 0.9), noise = (+0.2, -0.6): im_in = 0.7, clamp(1.1) = 1 / clamp(-0.1) = 0, 0.3, so
    mse_in = 0.04, 0.01 / 0.25, 0.36.  Clean x_hat = (0.4, 1.2 -> 1), pair x_hat = 0.6, 0.9 / -0.3 -> 0, 0.0, so
    mse_out = 0.04, 0.01 / 0.16, 1.0 and the dB values 0, 0 / 10 log10(0.64), 10 log10(1 / 0.36)."""
    im, noise = const([0.5, 0.9]), const([0.2, -0.6])
    clean, pairs = const([0.4, 1.2]), const([0.6, 0.9, -0.3, 0.0])
    im_in, mse_in = R.pair_inputs(im, noise)
    assert im_in.shape == (4, 3, 2, 4) and im_in.dtype == torch.float32
    assert torch.equal(im_in[1], torch.ones(3, 2, 4)) and torch.equal(im_in[2], torch.zeros(3, 2, 4))   # pair order
    close = lambda a, b: math.isclose(a, b, rel_tol=1e-6, abs_tol=1e-7)
    for got, want in zip(sum(mse_in, []), [0.04, 0.01, 0.25, 0.36]):
        assert close(got, want), (got, want)
    for got, want in zip(sum(R.pair_outputs(pairs, clean, 2, 2), []), [0.04, 0.01, 0.16, 1.0]):
        assert close(got, want), (got, want)
    for got, want in zip(sum(R.pair_outputs(pairs, clean, 2, 2, clamp=False), []), [0.04, 0.09, 0.49, 1.44]):
        assert close(got, want), (got, want)
    vi = R.pair_matrix(im, noise, pairs, clean)
    for got, want in zip(sum(vi, []), [0.0, 0.0, 10 * math.log10(0.64), 10 * math.log10(1 / 0.36)]):
        assert abs(got - want) < 1e-5, (got, want)


def test_restatement_cross_entry_is_the_mean_of_db_values():
    """mse_in = 0.01, 0.04 and mse_out = 0.1, 0.04: 10 dB and 0 dB, mean 5 (not the dB of the mean ratio, 3.2)."""
    im_s, im_adv = const([0.5, 0.5]), const([0.6, 0.3])
    out_s = const([0.2, 0.8])
    out_adv = const([0.2 + math.sqrt(0.1), 1.3])           # the second clamps to 1: (1 - 0.8)^2 = 0.04
    assert abs(R.cross_entry(im_s, im_adv, out_adv, out_s) - 5.0) < 1e-4


# --------------------------------------------------------------------------- #
# chunking
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("N,M,batch", [(1, 1, 32), (5, 3, 4), (3, 40, 32), (24, 24, 32)])
def test_pair_chunks(T, N, M, batch):
    chunks = T.pair_chunks(N, M, batch)
    seen = []
    for (i0, i1), (j0, j1) in chunks:
        n, m = i1 - i0, j1 - j0
        assert 0 <= i0 < i1 <= N and 0 <= j0 < j1 <= M
        assert n * m <= batch and m <= batch
        assert n == min(max(1, batch // m), N - i0)              # as many noises as fit beside the run of targets
        # the kernels put pair (a, b) of a block at a * m + b: noise-major, so ascending in i * M + j
        block = [(i0 + k // m) * M + j0 + k % m for k in range(n * m)]
        assert block == sorted(block)
        seen += block
    assert sorted(seen) == list(range(N * M))                     # every pair exactly once
    runs = list(dict.fromkeys(c[1] for c in chunks))
    assert [c[1] for c in chunks] == sorted(c[1] for c in chunks)  # a run's chunks are consecutive: one clean forward
    assert len(runs) == -(-M // batch)
    if (N, M, batch) == (5, 3, 4):
        assert chunks == [((i, i + 1), (0, 3)) for i in range(5)]
    if (N, M, batch) == (3, 40, 32):
        assert chunks == [((i, i + 1), (0, 32)) for i in range(3)] + [((0, 3), (32, 40))]
    if (N, M, batch) == (24, 24, 32):
        assert len(chunks) == 24


def test_pair_chunks_rejects_bad_counts(T):
    for bad in [(0, 1, 4), (1, 0, 4), (1, 1, 0), (1.0, 1, 4), (True, 1, 4)]:
        with pytest.raises(ValueError):
            T.pair_chunks(*bad)


# --------------------------------------------------------------------------- #
# the NaN rules
# --------------------------------------------------------------------------- #
def test_vi_db_guard(T):
    assert T.vi_db(1e-4, 1e-2) == 10.0 * math.log10(1e-2 / 1e-4)
    assert T.vi_db(1e-3, 1e-3) == 0.0
    for mi, mo in [(0.0, 1e-3), (1e-3, 0.0), (1e-20, 1e-3), (1e-3, 1e-20), (0.0, 0.0), (float("nan"), 1e-3)]:
        assert math.isnan(T.vi_db(mi, mo)), (mi, mo)
    assert math.isfinite(T.vi_db(1.1e-20, 1.1e-20))


def test_mismatched_sizes_are_nan(T):
    src = [(64, 64), (64, 128), (64, 64)]
    dst = [(64, 128), (64, 64), (128, 64), (64, 64)]
    blocks, mismatched = T.size_blocks(src, dst)
    assert blocks == [([0, 2], [1, 3]), ([1], [0])] and mismatched == 12 - 5
    full = T.assemble(3, 4, blocks, [[[1.0, 2.0], [3.0, 4.0]], [[5.0]]])
    want = [[None, 1.0, None, 2.0], [5.0, None, None, None], [None, 3.0, None, 4.0]]
    for i in range(3):
        for j in range(4):
            assert math.isnan(full[i][j]) if want[i][j] is None else full[i][j] == want[i][j], (i, j)
    assert T.size_blocks([(64, 64)], [(128, 128)]) == ([], 1)
    assert T.size_blocks([(64, 64)] * 2, [(64, 64)] * 3) == ([([0, 1], [0, 1, 2])], 0)


# --------------------------------------------------------------------------- #
# argument checks: refused before any launch (no device is touched)
# --------------------------------------------------------------------------- #
def test_bad_shapes_raise_value_error(T):
    with pytest.raises(ValueError):
        T.apply_pairs(torch.zeros(3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        T.apply_pairs(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(ValueError):
        T.score_pairs(torch.zeros(2, 3, 8, 8), torch.zeros(2, 1, 8, 8, 4), 1, 2)
    with pytest.raises(ValueError):
        T.score_pairs(torch.zeros(2, 1, 8, 8, 4), torch.zeros(2, 1, 8, 8, 4), 0, 2)
    with pytest.raises(ValueError):
        T.transfer_matrix(None, torch.zeros(1, 3, 8, 8), torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError):
        T.apply_pairs(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))       # a CPU tensor: there is no CPU path


# --------------------------------------------------------------------------- #
# the CLI's parser
# --------------------------------------------------------------------------- #
def test_cli_parser(TN):
    parse = TN.config().parse_args
    a = parse(["-m", "hyper", "-q", "3", "-s2", "src/*.png", "-s", "dst/*.png"])
    assert (a.source2, a.source, a.cross_model) == ("src/*.png", "dst/*.png", False)
    assert TN.matrix_file_name(a) == "hyper_3_ms-ssim_transfer.pkl"
    assert parse(["--source2", "x.png"]).source2 == "x.png" and parse([]).source2 is None
    a = parse(["--cross-model"])
    assert a.cross_model and a.models == "factorized,hyper,context,cheng2020"
    assert TN.model_list(a) == ["factorized", "hyper", "context", "cheng2020"]
    a = parse(["--cross-model", "--models", "factorized, hyper", "-metric", "mse", "-q", "1"])
    assert TN.model_list(a) == ["factorized", "hyper"] and TN.CROSS_FILE == "transfer_methods.npy"
    with pytest.raises(ValueError):
        TN.model_list(parse(["--cross-model", "--models", ","]))
    with pytest.raises(SystemExit):
        parse(["-model2", "1"])                      # not offered: the reference's flag never did anything
    with pytest.raises(ValueError):
        TN.main(["-s", "dst/*.png"])                 # neither -s2 nor --cross-model
    # every reference flag of coder.config() is still there
    a = parse(["-steps", "3", "--batch", "4", "--synthetic-weights", "-noise", "1e-3"])
    assert (a.steps, a.batch, a.synthetic_weights, a.noise) == (3, 4, True, 1e-3)
