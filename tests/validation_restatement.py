"""The trainer's validation (validate.py, the reference's test_epoch, train.py:196-242) restated with oracle.codec
functions, oracle.attack.attack, oracle.msssim and torch, following the dtype it is given; plus the cases and bounds
of the ica_val_metrics kernel's tests.

Plain, per image (train.RateDistortionLoss(training=True) with N = 1 on codec.forward(training=False)):

    bpp        = sum over the likelihood tensors of  sum ln max(lik, 2^-16) / (-ln 2 * H * W)
    distortion = mean((x_hat - target)^2), x_hat NOT clamped            (-metric mse)
               = pytorch_msssim.ms_ssim(x_hat, target), x_hat NOT clamped (-metric ms-ssim)
    loss       = lambda * 255^2 * mse + lamb_r * bpp   or   lambda * (1 - msim) + lamb_r * bpp;  lamb_r = 0 at lambda 100

--adv, per image: vi = 10 log10(mse_out / mse_in) of oracle.attack.attack(noise_thr=1e-4, per-image semantics).

Kernel bound (kernel_tol): the form tests/rd_eval_restatement.py KERNEL_TOL has, 4 max(e_ref, 2^-24) rounded up to one
digit, with e_ref measured in the test: the distance of this restatement in fp32 from itself in float64 on the same
inputs (rel_err = max |a - b| / max |b| over the batch).  2^-24 is one fp32 rounding.

Composition bounds: FORWARD_TOL of tests/rd_eval_restatement.py (bpp and mse relative 1e-3, msim absolute 1e-5), and
what follows from them for the loss, every term being positive:

    mse:      |d loss| <= 1e-3 * (lambda 255^2 mse + bpp) = 1e-3 * loss
    ms-ssim:  |d loss| <= lambda * 1e-5 + 1e-3 * bpp

VI bound: tests/test_gpu_attack.py holds the short trajectories' mse_in to a relative 1e-3 (test_attack_vs_oracle_256);
mse_out is a mean of the same kind over the reconstructions, held to the same 1e-3 by FORWARD_TOL.  Then
|d vi| = 10 |log10((mse_out' / mse_out) / (mse_in' / mse_in))| <= 10 log10((1 + 1e-3) / (1 - 1e-3)) = 8.69e-3 dB.
"""
import math

import torch

from oracle import attack as oattack
from oracle import codec
from oracle import msssim as omsssim
from tests import rd_eval_restatement as RD

LIK_MIN = RD.LIK_MIN
VAL_NOISE = 1e-4
VI_TOL = 10.0 * math.log10((1 + 1e-3) / (1 - 1e-3))


# --------------------------------------------------------------------------- #
# Restatement
# --------------------------------------------------------------------------- #
def kernel_ref(x_hat, target, lik_y, lik_z=None, dtype=torch.float64):
    """(sse [B], lny [B], lnz [B]) in dtype; x_hat is not clamped."""
    sse = ((x_hat.to(dtype) - target.to(dtype)) ** 2).flatten(1).sum(1)

    def plane(lik):
        if lik is None:
            return torch.zeros(x_hat.shape[0], dtype=dtype)
        return torch.log(torch.clamp(lik.to(dtype), min=LIK_MIN)).flatten(1).sum(1)

    return sse, plane(lik_y), plane(lik_z)


def loss_terms(output, target, metric, lmbda):
    """Per-image RateDistortionLoss(output, target, training=True), N = 1, in the dtype of ``output``: a dict of [B]
    tensors loss / bpp / distortion."""
    B, _, H, W = target.shape
    liks = output["likelihoods"]
    dtype = output["x_hat"].dtype
    sse, lny, lnz = kernel_ref(output["x_hat"], target, liks["y"], liks.get("z"), dtype)
    den = -math.log(2) * (H * W)
    bpp = lny / den + lnz / den
    lamb_r = 0.0 if lmbda == 100 else 1.0
    if metric == "mse":
        dist = sse / (3 * H * W)
        loss = lmbda * 255 ** 2 * dist + lamb_r * bpp
    else:
        dist = omsssim.ms_ssim_per_image(output["x_hat"], target.to(dtype))
        loss = lmbda * (1 - dist) + lamb_r * bpp
    return {"loss": loss, "bpp": bpp, "distortion": dist}


def plain(P, x, model, metric, lmbda, dtype=torch.float64):
    """train.py:217-229 per image: criterion(net.eval()(d), d, training=True)."""
    with torch.no_grad():
        out = codec.forward(RD.to_dtype(P, dtype), x.to(dtype), model, training=False)
        return loss_terms(out, x.to(dtype), metric, lmbda)


def adv_vi(P, x, steps, model="hyper", dtype=torch.float32, **kw):
    """train.py:210-215 per image: the VI list of the attack at noise 1e-4 (None where it is undefined)."""
    ref = oattack.attack(RD.to_dtype(P, dtype), x.to(dtype), steps=steps, noise_thr=VAL_NOISE, model=model,
                         coupled=False, eval_msssim=False, **kw)
    return ref.eval.vi


def mean64(values):
    """The float64 sum of the values, in order, over their number."""
    s = torch.zeros((), dtype=torch.float64)
    for v in values:
        s = s + torch.tensor(v, dtype=torch.float64)
    return float(s / len(values))


def log_line(epoch, loss, d, bpp, recomp=0.0):
    """train.py:233's format string."""
    return (f"Test epoch {epoch}: Average losses:\tLoss: {loss:.4f} |\tMSE loss: {d:.6f} |\tBpp loss: {bpp:.3f} |"
            f"\tRecomp loss: {recomp:.3f}\n")


# --------------------------------------------------------------------------- #
# Kernel cases: (image shape, y likelihood shape, z likelihood shape or None) at the latent sizes of the 64x64 and
# 64x128 validation images (y at 1/16, z at 1/64: a z plane of one element), B = 1 and 3, both channel pairs, and the
# factorized model (no z).  The tensors are RD.kernel_case's: x_hat in [-0.3, 1.3] with values planted below 0 and
# above 1 (a clamped implementation fails), likelihoods planted exactly at 2^-16, next to it on both sides and at 1e-9.
# --------------------------------------------------------------------------- #
KERNEL_CASES = [
    ((1, 3, 64, 64), (1, 192, 4, 4), (1, 128, 1, 1)),
    ((3, 3, 64, 64), (3, 192, 4, 4), (3, 128, 1, 1)),
    ((3, 3, 64, 128), (3, 320, 4, 8), (3, 192, 1, 2)),
    ((1, 3, 64, 128), (1, 192, 4, 8), None),
    ((3, 3, 64, 64), (3, 320, 4, 4), None),
]


def round_up_1(v):
    """v rounded up to one significant digit (2.38e-7 -> 3e-7), as KERNEL_TOL's entries are."""
    e = math.floor(math.log10(v))
    return math.ceil(v / 10 ** e - 1e-12) * 10 ** e


def kernel_tol(e_ref):
    """{sum: bound} from the fp32 restatement's own errors; a sum that is exactly 0 (no z plane) has bound 0."""
    return {k: (0.0 if v == 0.0 else round_up_1(4 * max(v, 2.0 ** -24))) for k, v in e_ref.items()}


# --------------------------------------------------------------------------- #
# Composition cases
# --------------------------------------------------------------------------- #
def plain_params(model, quality=1):
    """The synthetic weights as the train tests perturb them."""
    return codec.perturb_params(codec.init_params(model, quality, seed=0), seed=1)


def adv_params(quality=1):
    """... with g_a's last layer scaled by 40 (tests/test_gpu_attack.py): |y| ~ 1, the eval reconstruction moves under
    the attack and the VI is defined."""
    P = plain_params("hyper", quality)
    P["g_a.6.weight"] = P["g_a.6.weight"] * 40.0
    return P


# Two 64x64 images for which the float64 oracle's VI after 3 steps is defined and the fp32 oracle's agrees with it to
# a tenth of VI_TOL (checked in tests/test_cpu_validation.py): the case is one fp32 arithmetic can settle.
ADV_SEED, ADV_STEPS, ADV_SHAPE = 211, 3, (2, 3, 64, 64)


def image8(shape, seed):
    """A seeded image on the 8-bit grid, as a PNG round trip gives it."""
    return torch.round(RD.image(shape, seed) * 255.0) / 255.0
