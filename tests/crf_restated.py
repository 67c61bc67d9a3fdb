"""The dense-CRF boundary refinement restated in torch, by brute force in fp64 (or, for the tests' error bars, in fp32): the rule of
ReID_net/scripts/postproc/crf/crf_davis.py:43-60 (``apply_crf``) with densecrf's defaults -- Potts compatibility, symmetric normalisation,
``-unary - pairwise`` -- but with the Gaussian filters computed EXACTLY over a truncated square window instead of on the permutohedral
lattice.  Written from the rule, not from the kernels (csrc/crf_ops.hip), which are held to it.

    pair weight   k_g(i,j) = exp(-(dy^2 + dx^2) / (2 sxy_g^2))                                   |dy|, |dx| <= R_g, the centre included
                  k_b(i,j) = exp(-(dy^2 + dx^2) / (2 sxy_b^2) - |I_i - I_j|^2 / (2 srgb^2))      |dy|, |dx| <= R_b
                  window positions outside the image do not exist
    normaliser    n_m(i) = 1 / sqrt(sum_j k_m(i,j) + 1e-20)
    iteration     Q^0 = softmax_l(-U);  Q~_m[l,i] = n_m(i) sum_j k_m(i,j) n_m(j) Q[l,j];  Q <- softmax_l(-U + sum_m w_m Q~_m)
    output        argmax_l Q, a tie to the lowest label
    unary         U[l,i] = -log(p) where l is pixel i's label, -log((1 - p) / (L - 1)) elsewhere   (pydensecrf unary_from_labels)

Every pair weight of a frame is held as one dense [P,P] matrix (P = H W pixels, zero outside the window), built in row blocks: fine for
the tests' frames (P <= 10 500, 0.9 GB in fp64), not meant for anything larger."""
import math

import torch

DEFAULTS = {"sxy": 22.3761305044, "srgb": 7.70254062277, "compat": 1.40326787165, "gsxy": 0.220880737269, "gcompat": 1.24845093352,
            "r": 56, "gr": 1, "iters": 12, "gt_prob": 0.7}                                       # crf_davis.py:43-60; r = ceil(2.5 sxy)
ROW_BLOCK = 256


def params(**given):
    """``DEFAULTS`` with ``given`` on top; ``r`` / ``gr`` follow their sigma when only the sigma is given."""
    p = dict(DEFAULTS, **given)
    if "sxy" in given and "r" not in given:
        p["r"] = math.ceil(2.5 * p["sxy"])
    if "gsxy" in given and "gr" not in given:
        p["gr"] = max(1, math.ceil(2.5 * p["gsxy"]))
    return p


def unary_from_labels(idmap, L, gt_prob, dtype=torch.float64):
    """uint8 [H,W] -> U [L,H,W]."""
    lab = torch.as_tensor(idmap).long()
    assert int(lab.max()) < L
    p = torch.tensor(gt_prob, dtype=dtype)
    U = (-torch.log((1 - p) / (L - 1))).expand(L, *lab.shape).clone()
    U.scatter_(0, lab[None], (-torch.log(p)).expand(1, *lab.shape))
    return U


def pair_weights(frame, sxy, srgb, R, dtype=torch.float64):
    """uint8 [H,W,3] -> K [P,P], K[i,j] = k(i,j) inside the window of radius R around i and 0 elsewhere; ``srgb`` None: no colour term."""
    frame = torch.as_tensor(frame)
    H, W = frame.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ys, xs, col = ys.reshape(-1), xs.reshape(-1), frame.reshape(-1, 3).to(dtype)
    K = torch.empty((H * W, H * W), dtype=dtype)
    for a in range(0, H * W, ROW_BLOCK):
        b = min(a + ROW_BLOCK, H * W)
        dy, dx = ys[a:b, None] - ys[None], xs[a:b, None] - xs[None]
        e = (dy * dy + dx * dx).to(dtype) / (-2.0 * sxy * sxy)
        if srgb is not None:
            d2 = torch.zeros_like(e)
            for c in range(3):
                d = col[a:b, None, c] - col[None, :, c]
                d2 += d * d
            e = e - d2 / (2.0 * srgb * srgb)
        K[a:b] = torch.exp(e) * ((dy.abs() <= R) & (dx.abs() <= R))
    return K


def normaliser(K):
    return 1.0 / torch.sqrt(K.sum(1) + 1e-20)


def message(K, n, Q):
    """Q [L,P] -> Q~ [L,P]."""
    return n * ((n * Q) @ K.T)


def meanfield(frame, U, p, dtype=torch.float64):
    """frame uint8 [H,W,3], U [L,H,W], p: ``params()`` -> {"n_g", "n_b" [H,W], "Q0", "Q1" (after round 1), "Q" (after the last) [L,H,W]}."""
    L, H, W = U.shape
    U = torch.as_tensor(U).to(dtype).reshape(L, -1)
    Kg = pair_weights(frame, p["gsxy"], None, p["gr"], dtype)
    Kb = pair_weights(frame, p["sxy"], p["srgb"], p["r"], dtype)
    ng, nb = normaliser(Kg), normaliser(Kb)
    Q = torch.softmax(-U, 0)
    out = {"n_g": ng.reshape(H, W), "n_b": nb.reshape(H, W), "Q0": Q.reshape(L, H, W)}
    for it in range(p["iters"]):
        Q = torch.softmax(-U + p["gcompat"] * message(Kg, ng, Q) + p["compat"] * message(Kb, nb, Q), 0)
        if it == 0:
            out["Q1"] = Q.reshape(L, H, W)
    out["Q"] = Q.reshape(L, H, W)
    return out


def labels_of(Q):
    """[L,H,W] -> uint8 [H,W]: the argmax, a tie to the lowest label."""
    best = Q.max(0).values
    lab = torch.zeros(Q.shape[1:], dtype=torch.uint8)
    for l in range(Q.shape[0] - 1, -1, -1):
        lab[Q[l] == best] = l
    return lab


def margin_of(Q):
    """[L,H,W] -> [H,W]: the gap between the two largest Q of a pixel."""
    top = Q.topk(2, 0).values
    return top[0] - top[1]


def refine(frame, idmap, L, p, dtype=torch.float64):
    """One frame, from an id map: ``meanfield``'s dict plus "U", "labels" uint8 [H,W], "changed" (pixels whose label differs from
    ``idmap``) and "margin" [H,W]."""
    U = unary_from_labels(idmap, L, p["gt_prob"], dtype)
    out = meanfield(frame, U, p, dtype)
    out["U"] = U
    out["labels"] = labels_of(out["Q"])
    out["changed"] = int((out["labels"] != torch.as_tensor(idmap)).sum())
    out["margin"] = margin_of(out["Q"])
    return out


def synthetic(H, W, L, seed, label_noise=0.03, sigma=5.0, shift=2):
    """The tests' seeded frame: piecewise-constant colour regions (a Voronoi partition, region r coloured from the seed and labelled
    r mod L), the label boundaries displaced ``shift`` px from the colour boundaries, Gaussian pixel noise of ``sigma``, and
    ``label_noise`` of the pixels given a random label -> (frame uint8 [H,W,3], idmap uint8 [H,W]); every label < L, label L - 1 present."""
    g = torch.Generator().manual_seed(seed)
    regions = max(L, 5)
    cy, cx = torch.rand(regions, generator=g) * H, torch.rand(regions, generator=g) * W
    colours = torch.randint(20, 236, (regions, 3), generator=g).double()
    ys, xs = torch.meshgrid(torch.arange(H).double(), torch.arange(W).double(), indexing="ij")

    def nearest(yy, xx):
        return ((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2).argmin(0)
    frame = colours[nearest(ys, xs)] + sigma * torch.randn((H, W, 3), generator=g).double()
    frame = frame.round().clamp(0, 255).to(torch.uint8)
    idmap = (nearest(ys + shift, xs + shift) % L).to(torch.uint8)
    flip = torch.rand((H, W), generator=g) < label_noise
    idmap[flip] = torch.randint(0, L, (int(flip.sum()),), generator=g).to(torch.uint8)
    idmap[0, 0] = L - 1
    return frame, idmap
