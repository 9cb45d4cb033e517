"""CPU restatement of the reference's latent-range code and the pinned inputs of tests/test_gpu_latent_range.py.

The reference's search.py cannot be imported (it pulls in lpips and matplotlib) and feature_range.py is a
script, so their few torch lines are restated here, each citing its source:

  ranges             feature_range.py:19-21
  channel_profile    feature_range.py:65-66
  clamp_value_naive  search.py:32-35 == attack_rd.py:64-67
  detect             search.py:137-146
  eval_defend_range  attack_rd.py:261-268, :302-311 (the eval with args.defend), per image
  clamp_expensive    g_s(clamp(g_a(.))) for oracle.attack.attack(expensive=...): the attack through the clamp (no
                     such loop exists in the reference; it is attack_our, attack_rd.py:340-349, with the clamp
                     inserted)
"""
import functools
import math

import torch

from oracle import attack as oa
from oracle import codec


def ranges(y):
    """feature_range.py:19-21 (without keepdim): [B][C] each."""
    return torch.amax(y, dim=(2, 3)), torch.amin(y, dim=(2, 3)), torch.amax(torch.abs(y), dim=(2, 3))


def channel_profile(index_max, index_min, topk=100):
    """feature_range.py:65-66 on [N][C] rows (the reference's are [N][C][1][1])."""
    channel_max = index_max.topk(k=topk, dim=0)[0][-1]
    channel_min = index_min.topk(k=topk, dim=0, largest=False)[0][-1]
    return channel_max, channel_min


def clamp_value_naive(y_main, channel_max, channel_min):
    """search.py:32-35."""
    channel_max = channel_max.view(1, -1, 1, 1)
    channel_min = channel_min.view(1, -1, 1, 1)
    y_main = torch.where(y_main > channel_max, channel_max, y_main)
    y_main = torch.where(y_main < channel_min, channel_min, y_main)
    return y_main


def detect_from_ranges(index_max, index_min, channel_max, channel_min):
    """search.py:143-146 for one image: index_max / index_min / channel_* are [C]."""
    err_max = torch.clamp(index_max - channel_max, min=0.0)
    err_min = torch.clamp(index_min - channel_min, max=0.0)
    return torch.max(err_max / (channel_max + 1)) + torch.max(torch.abs(err_min / (channel_min + 1)))


def detect(y_main, channel_max, channel_min):
    """search.py:137-146, one image ([1][C][H][W])."""
    channel_max = channel_max.view(1, -1, 1, 1)
    channel_min = channel_min.view(1, -1, 1, 1)
    index_max = torch.amax(y_main, dim=(2, 3), keepdim=True)
    index_min = torch.amin(y_main, dim=(2, 3), keepdim=True)
    err_max = torch.clamp(index_max - channel_max, min=0.0)
    err_min = torch.clamp(index_min - channel_min, max=0.0)
    return torch.max(err_max / (channel_max + 1)) + torch.max(torch.abs(err_min / (channel_min + 1)))


# --------------------------------------------------------------------------- #
# the oracle composition g_a -> where -> entropy model -> g_s(round)
# --------------------------------------------------------------------------- #
def analysis(P, x, model):
    return codec.cheng_g_a(P, x) if model == "cheng2020" else codec.g_a(P, x)


def synthesis(P, y, model):
    return codec.cheng_g_s(P, y) if model == "cheng2020" else codec.g_s(P, y)


def entropy_estimator(P, y, model):
    """anchors/model.py:86-108, eval mode: the likelihoods of y."""
    if model == "factorized":
        return {"y": codec.entropy_bottleneck(P, y)[1]}
    if model == "hyper":
        z_hat, z_lik = codec.entropy_bottleneck(P, codec.h_a(P, torch.abs(y)))
        return {"y": codec.gaussian_conditional(y, codec.h_s(P, z_hat))[1], "z": z_lik}
    h_a, h_s = (codec.cheng_h_a, codec.cheng_h_s) if model == "cheng2020" else (codec.mbt_h_a, codec.mbt_h_s)
    z_hat, z_lik = codec.entropy_bottleneck(P, h_a(P, y))
    ctx = codec.context_prediction(P, torch.round(y))
    scales, means = codec.entropy_parameters(P, torch.cat((h_s(P, z_hat), ctx), dim=1)).chunk(2, 1)
    return {"y": codec.gaussian_conditional(y, scales, means)[1], "z": z_lik}


def defended_forward(P, im_, channel_max, channel_min, model, clamp_latent=True):
    """attack_rd.py:264-268: (y_main after defend, likelihoods, output_).  clamp_latent=False leaves the defence
    out (the undefended composition, for the CPU check that a missing clamp cannot pass)."""
    with torch.no_grad():
        y = analysis(P, im_, model)
        yc = clamp_value_naive(y, channel_max, channel_min) if clamp_latent else y
        lik = entropy_estimator(P, yc, model)
        out = torch.clamp(synthesis(P, torch.round(yc), model), min=0.0, max=1.0)
    return y, yc, lik, out


def eval_defend_range(P, im_adv, im_s, output_s, channel_max, channel_min, model="hyper", clamp=True):
    """The reference's eval with args.defend (attack_rd.py:238, :261-268, :302-311), per image."""
    B, _, H, W = im_adv.shape
    im_ = torch.clamp(im_adv, 0.0, 1.0) if clamp else im_adv
    y, yc, lik, out = defended_forward(P, im_, channel_max, channel_min, model)
    results = []
    for b in range(B):
        mi = float(torch.mean((im_[b] - im_s[b]) ** 2))
        mo = float(torch.mean((out[b] - output_s[b]) ** 2))
        r = {"bpp": float(codec.bpp({k: v[b:b + 1] for k, v in lik.items()}, H * W)), "mse_in": mi, "mse_out": mo,
             "vi": 10.0 * math.log10(mo / mi) if mi > 1e-20 and mo > 1e-20 else None,
             "nclamped": int((yc[b] != y[b]).sum())}
        results.append(r)
    return results, out, y, yc


def clamp_expensive(P, channel_max, channel_min, dtype=torch.float32):
    """f(im_in, step) -> g_s(clamp_value_naive(g_a(im_in))) with the network in `dtype` (float64: the replay that
    measures the restatement's own sensitivity to network rounding, as tests/cw_restatement.reference_error)."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    cmax, cmin = channel_max.to(dtype), channel_min.to(dtype)

    def f(x, step):
        y = clamp_value_naive(codec.g_a(Pd, x.to(dtype)), cmax, cmin)
        return codec.g_s(Pd, y).to(x.dtype)
    return f


# --------------------------------------------------------------------------- #
# pinned inputs
# --------------------------------------------------------------------------- #
def rnd(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


# The profile of a pinned case is the clean images' own per-channel range times this.  0.5 clamps 26-38 % of the
# latent of the bmshj2018 / mbt2018 cases; cheng2020's latent has 20 channels whose maximum is <= 0 and 21 whose
# minimum is >= 0 (a bound of such a channel moves towards 0 and past the data), so 0.5 clamps 53.4 % there, over
# the 50 % the inputs are held to, and 0.7 is used (27.7 %).
PROFILE_SCALE = {"hyper": 0.5, "factorized": 0.5, "context": 0.5, "cheng2020": 0.7}
EVAL_SHAPES = {"hyper": (2, 3, 128, 192), "factorized": (2, 3, 128, 192), "context": (1, 3, 64, 128),
               "cheng2020": (1, 3, 64, 128)}
EVAL_QUALITY = {"hyper": 3, "factorized": 3, "context": 3, "cheng2020": 3}


@functools.lru_cache(maxsize=None)
def eval_params(model):
    P = codec.perturb_params(codec.init_params(model, EVAL_QUALITY[model], seed=0), seed=1)
    # |y| ~ 1 and more: the rounded-latent reconstructions move
    P["g_a.6.weight"] = P["g_a.6.weight"] * (10.0 if model == "cheng2020" else 40.0)
    return P


def own_profile(P, im_s, model, scale=None):
    """The profile of the pinned tests: the clean images' own per-channel range over the batch, times `scale`
    (default: the model's PROFILE_SCALE)."""
    scale = PROFILE_SCALE[model] if scale is None else scale
    with torch.no_grad():
        y = analysis(P, im_s, model)
    return torch.amax(y, dim=(0, 2, 3)) * scale, torch.amin(y, dim=(0, 2, 3)) * scale


@functools.lru_cache(maxsize=None)
def eval_case(model):
    """(P, im_adv, im_s, output_s, channel_max, channel_min) of the defended-eval comparison."""
    P = eval_params(model)
    shape = EVAL_SHAPES[model]
    im_s = rnd(shape, 21)
    im_adv = (im_s + rnd(shape, 22, -0.05, 0.05)).clamp(0, 1)
    with torch.no_grad():
        output_s = codec.forward(P, im_s, model)["x_hat"].clamp(0, 1)
    cmax, cmin = own_profile(P, im_s, model)
    return P, im_adv, im_s, output_s, cmax, cmin


@functools.lru_cache(maxsize=None)
def eval_reference(model):
    P, im_adv, im_s, output_s, cmax, cmin = eval_case(model)
    return eval_defend_range(P, im_adv, im_s, output_s, cmax, cmin, model)


ADV_STEPS, ADV_THR, ADV_LR = 8, 1e-3, 0.01


@functools.lru_cache(maxsize=None)
def adv_case():
    """(P, x[3], channel_max, channel_min) of the attack-through-clamp trajectory: hyper q3, 64x64; the GPU test
    attacks x[:2] as a batch, and x[1] inside the batch of 3 and alone."""
    P = eval_params("hyper")
    x = rnd((3, 3, 64, 64), 70)
    cmax, cmin = own_profile(P, x, "hyper")
    return P, x, cmax, cmin


@functools.lru_cache(maxsize=None)
def adv_reference(n=2, dtype=torch.float32):
    P, x, cmax, cmin = adv_case()
    rec = []
    ref = oa.attack(P, x[:n], steps=ADV_STEPS, noise_thr=ADV_THR, lr=ADV_LR, eval_msssim=False, record=rec, adv=True,
                    expensive=clamp_expensive(P, cmax, cmin, dtype))
    return ref, rec
