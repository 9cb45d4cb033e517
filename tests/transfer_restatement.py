"""Plain-torch CPU restatement of transfer_noise.py's two studies, with float64 metrics from given reconstructions:
the oracle of tests/test_cpu_transfer.py and tests/test_gpu_transfer.py.

pair_inputs     test (transfer_noise.py:88-89): clamp(im[j] + noise[i], 0, 1) and mean((im_in - im[j])^2) per pair
pair_outputs    transfer_noise.py:96, :133: mean((clamp(x_hat(im_in)) - clamp(x_hat(im)))^2) per pair
pair_matrix     the double loop (transfer_noise.py:117-135): 10 log10(mse_out / mse_in), source-major
cross_entry     test_transferability_multiple_models (transfer_noise.py:63-77): one entry of the model matrix

Pair (i, j) of N noises and M images sits at index i * M + j.  The codec is not restated: reconstructions come in.
"""
import math

import torch


def rand_image(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def pair_inputs(im, noise):
    """(im_in [N M, 3, H, W] in the dtype of im, mse_in [N][M] float64 list) for im [M, ...] and noise [N, ...]."""
    N, M = noise.shape[0], im.shape[0]
    im_in, mse = [], [[0.0] * M for _ in range(N)]
    for i in range(N):
        for j in range(M):
            x = torch.clamp(im[j] + noise[i], min=0.0, max=1.0)
            im_in.append(x)
            mse[i][j] = float(((x.double() - im[j].double()) ** 2).mean())
    return torch.stack(im_in), mse


def pair_outputs(x_hat_pairs, x_hat_clean, N, M, clamp=True):
    """mse_out [N][M] float64 list from the reconstructions x_hat_pairs [N M, 3, H, W] and x_hat_clean [M, 3, H, W]."""
    c = (lambda t: t.clamp(0.0, 1.0)) if clamp else (lambda t: t)
    a, s = c(x_hat_pairs.double()), c(x_hat_clean.double())
    return [[float(((a[i * M + j] - s[j]) ** 2).mean()) for j in range(M)] for i in range(N)]


def db(mse_in, mse_out):
    return 10 * math.log10(mse_out / mse_in)


def pair_matrix(im, noise, x_hat_pairs, x_hat_clean, clamp=True):
    """[N][M] dB values of the -s2 loop."""
    N, M = noise.shape[0], im.shape[0]
    _, mse_in = pair_inputs(im, noise)
    mse_out = pair_outputs(x_hat_pairs, x_hat_clean, N, M, clamp)
    return [[db(mse_in[i][j], mse_out[i][j]) for j in range(M)] for i in range(N)]


def cross_entry(im_s, im_adv, out_adv, out_s):
    """Mean over the images of 10 log10(mean((c(out_adv) - c(out_s))^2) / mean((im_s - im_adv)^2)), c = clamp to
    [0, 1]: entry [a][b] from model a's adversarial examples and model b's reconstructions."""
    vals = []
    for b in range(im_s.shape[0]):
        mse_in = float(((im_s[b].double() - im_adv[b].double()) ** 2).mean())
        d = out_adv[b].double().clamp(0.0, 1.0) - out_s[b].double().clamp(0.0, 1.0)
        vals.append(db(mse_in, float((d ** 2).mean())))
    return sum(vals) / len(vals)
