"""Drop-in for transfer_noise.py: does a perturbation found on image A also break image B, and does an adversarial
example found on model A also break model B?

    python -m imagecompression_adversarial_amd.transfer_noise -m hyper -q 3 -s2 'src/*.png' -s 'dst/*.png'
    python -m imagecompression_adversarial_amd.transfer_noise -q 3 --cross-model -s 'kodim*.png'
    python -m imagecompression_adversarial_amd.transfer_noise -m hyper -q 1 --synthetic-weights \
        -s2 synthetic:2x64x64 -s synthetic:3x64x64

test, the -s2 loop                    transfer_noise.py:83-96, :110-151   transfer.transfer_matrix (ica_transfer.hip)
test_transferability_multiple_models  transfer_noise.py:45-79, :153-175   transfer.cross_model_matrix

Differences from the reference, all deliberate (DESIGN.md "Transfer"):
  * The matrix is N x M, the numbers of -s2 and -s images, not the hard-coded 24 x 24.
  * Pairs whose padded sizes differ are NaN, and one line says how many (the reference raises on the size mismatch,
    e.g. on Kodak's portrait images).  A pair whose mse_in or mse_out is not above 1e-20 is NaN as well.
  * The clean reconstruction of a target is computed once, not once per pair; the -s2 images are attacked
    ``--batch`` at a time and the pairs are coded ``--batch`` at a time, with per-image semantics.
  * The three fixed-name PNGs the reference overwrites on every iteration (and the transfer_*.png of --debug) and
    the matplotlib figures are not written.
  * ``--cross-model`` computes what the reference's commented-out block computes (over ``--models`` at ``-q``) and
    saves it to transfer_methods.npy; the reference only plots a file saved earlier.
  * ``-model2`` is not offered: the reference's help text promises a second checkpoint but the flag is an int that
    only ever raised NotImplementedError.
"""
from __future__ import annotations

import torch

from . import attack_rd, coder, transfer

CROSS_MODELS = "factorized,hyper,context,cheng2020"     # transfer_noise.py:164
CROSS_FILE = "transfer_methods.npy"                     # transfer_noise.py:173


def config():
    p = coder.config()
    p.add_argument("-s2", "--source2", type=str, default=None,
                   help="images the perturbations are found on (glob, or synthetic:<B>x<H>x<W>)")
    p.add_argument("--cross-model", action="store_true", help="cross-model transferability over --models")
    p.add_argument("--models", type=str, default=CROSS_MODELS, help="comma list of the models --cross-model compares")
    return p


def model_list(args):
    names = [m.strip() for m in args.models.split(",") if m.strip()]
    if not names:
        raise ValueError("--models names no model")
    return names


def matrix_file_name(args):
    return f"{args.model}_{args.quality}_{args.metric}_transfer.pkl"     # transfer_noise.py:112, :141


def _load(items, device):
    ims = [t if t is not None else coder.read_image(name)[0] for name, t, _, _ in items]
    return torch.cat(ims, 0).to(device).contiguous()


def _net(args):
    net = coder.load_model(args, training=False).to(args.device)
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _kern(net, args):
    return net.kernels(net.attack_precision(getattr(args, "precision", None)))


def _sizes(items):
    return [attack_rd._padded_shape(it)[2:] for it in items]


def noise_transfer(args):
    """-s2: attack the -s2 images, add each perturbation to each -s image (transfer_noise.py:110-151).  Returns the
    [N, M] matrix of dB values it saves."""
    print("[Noise Transfer]:", args.source2, "to", args.source)
    src, dst = attack_rd._sources(args.source2), attack_rd._sources(args.source)
    if not src or not dst:
        raise ValueError(f"no image matches {'-s2 ' + repr(args.source2) if not src else '-s ' + repr(args.source)}")
    net = _net(args)
    kern = _kern(net, args)
    N, M = len(src), len(dst)
    print(torch.Size((N, M)))
    noises = []
    for group in attack_rd._groups(src, args.batch):
        im_s = _load(group, args.device)
        im_adv = attack_rd.attack_(im_s, net, args)[0]
        noises += list((im_adv - im_s).split(1))
    blocks, mismatched = transfer.size_blocks(_sizes(src), _sizes(dst))
    parts = []
    for rows, cols in blocks:
        nz = torch.cat([noises[i] for i in rows], 0).contiguous()
        im = _load([dst[j] for j in cols], args.device)
        parts.append(transfer.transfer_matrix(kern, nz, im, max(args.batch, 1), args.clamp).vi)
    full = transfer.assemble(N, M, blocks, parts)
    for row in full:
        for v in row:
            print(v)                                     # transfer_noise.py:134: source-major, target-minor
    vis = torch.tensor(full, dtype=torch.float32)        # the dtype of the reference's torch.zeros(24, 24)
    if mismatched:
        print(f"[SIZE] {mismatched} of {N * M} pairs have different padded sizes: NaN")
    torch.save(vis, matrix_file_name(args))
    print(vis)
    return vis


def cross_model(args):
    """--cross-model: the [K, K] matrix over --models at -q (transfer_noise.py:45-79 and the block at :154-173)."""
    import numpy as np
    names = model_list(args)
    items = attack_rd._sources(args.source)
    if not items:
        raise ValueError(f"no image matches -s {args.source!r}")
    nets = []
    for name in names:
        args.model = name
        nets.append(_net(args))
    kerns = [_kern(net, args) for net in nets]
    net_of = {id(kern): net for kern, net in zip(kerns, nets)}
    images = [_load(group, args.device) for group in attack_rd._groups(items, len(items))]

    def attack_fn(kern, im_s):
        return attack_rd.attack_(im_s, net_of[id(kern)], args)[0]

    matrix = np.array(transfer.cross_model_matrix(kerns, attack_fn, images, max(args.batch, 1)))
    print("Transferability matrix:")
    print(matrix)
    np.save(CROSS_FILE, matrix)
    return matrix


def main(argv=None):
    args = config().parse_args(argv)
    if not args.source2 and not args.cross_model:
        raise ValueError("nothing to do: give -s2 <images> (noise transfer) or --cross-model")
    out = {}
    if args.source2:
        out["transfer"] = noise_transfer(args)
    if args.cross_model:
        out["cross_model"] = cross_model(args)
    return out[next(iter(out))] if len(out) == 1 else out


if __name__ == "__main__":
    main()
