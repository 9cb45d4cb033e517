"""The batch reduction of the universal perturbation's update (ica_universal.hip, steps 2-3 of its pinned order),
restated in torch fp32 on the CPU with exact ops: elementwise sub / mul / add are IEEE round-to-nearest, the masks
are torch.where(cond, g, g * 0), and the sum over the images is a Python loop of adds in the kernel's order.
tests/test_cpu_universal.py ties it to the reference's clamp autograd in float64."""
import torch


def masked_sum(noise, im_s, gnet, cheap, eps, gscale):
    """noise [1, 3, H, W], im_s [B, 3, H, W], gnet [B, 3, H, W] (the network gradient, read when not cheap) ->
    G [1, 3, H, W] = ((g_0 + g_1) + ...) + g_{B-1}, g_b the gradient of image b behind its own [0, 1] pass-through."""
    eps = torch.tensor(eps, dtype=noise.dtype)
    gscale = torch.tensor(gscale, dtype=noise.dtype)
    nc = torch.minimum(torch.maximum(noise, -eps), eps)
    G = None
    for b in range(im_s.shape[0]):
        s = im_s[b:b + 1]
        u = s + nc
        lowU = torch.clamp(u, min=0.0)
        ii = torch.clamp(lowU, max=1.0)
        if cheap:
            t = gscale * (s - ii)
            g = -(t + t)
        else:
            g = gnet[b:b + 1]
        g = torch.where((lowU <= 1.0) | (g > 0.0), g, g * 0.0)   # Up_bound backward
        g = torch.where((u >= 0.0) | (g < 0.0), g, g * 0.0)      # Low_bound backward
        G = g if G is None else G + g
    return G


def im_in_of(noise, im_s, eps):
    """clamp(im_s + clamp(noise, -eps, eps), 0, 1) in the dtype of its operands."""
    return torch.clamp(im_s + torch.clamp(noise, -eps, eps), 0.0, 1.0)
