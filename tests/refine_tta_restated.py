"""The test-time augmentation rule of the refinement net, restated in a few lines of torch on the CPU from the oracle's pieces
(oracle/refinement_oracle.py: make_input, resize_bilinear_tf, deeplab_logits, resize_nearest_tf, conf_score).  TEST INFRASTRUCTURE:
it imports nothing from the product; the kernels (csrc/refine_ops.hip: tta_input_kernel, tta_softmax_kernel) and the plan
(refinement/model.py) are held to it.

The rule, each step with the reference line it restates (refinement_net/network/deeplab/model.py, predict_labels_multi_scale
:84-160, the scale handling :200-325).  A spec is a list of scales plus a flip flag ("0.75,1,1.25+flip"); the members, in order: per
scale as listed the unmirrored crop, then (flip) the mirrored one.  For a box with plain network input x [S,S,4], S = 385:
  1. S_s = scale_dimension(S, s); x_s = the align_corners=True bilinear resize of x to S_s x S_s, all four channels (:272-277);
     s = 1: the identity
  2. the mirrored member is x_s reversed along the width (tf.reverse_v2(images, [2]), :118)
  3. the net body on the member: logits on its native grid scale_dimension(S_s, 0.25)
  4. resized with align_corners=True to L x L, L = scale_dimension(S, max(1, s) / 4) (:258-297); the identity for s >= 1
  5. a mirrored member's L x L logits are reversed along the width (:137), before any further resize
  6. L x L -> S x S by the resize SegmentationSoftmax itself uses (TF-legacy bilinear, SegmentationOutputLayers.py:35-61), NOT
     predict_labels_multi_scale's align-corners one: the output layer the weights were trained under; with the single member
     (1.0, unmirrored) the result is then plain inference exactly
  7. two-class softmax per pixel; P1 = the mean over the members of p1, P0 of p0 (:143-147), fp32 sums in member order, then / M;
     prob = P1, cls = 1 iff P1 > P0 (a tie: class 0, like tf.argmax)
  8. from prob / cls on: un-crop, zero padding and conf_score as without augmentation
"""
import numpy as np
import torch

from oracle import refinement_oracle as R


def spec_of(spec):
    """"0.75,1+flip" (or an object with ``scales`` / ``flip``) -> ([0.75, 1.0], True)."""
    if isinstance(spec, str):
        body, _, tail = spec.partition("+")
        return [float(t) for t in body.split(",")], tail == "flip"
    return [float(s) for s in spec.scales], bool(spec.flip)


def member_table(spec, S=R.INPUT_SIZE):
    """(scale, S_s, L, mirrored) per member, in member order."""
    scales, flip = spec_of(spec)
    return [(s, R.scale_dimension(S, s), R.scale_dimension(S, max(1.0, s) / 4.0), m) for s in scales for m in ((False, True) if flip else (False,))]


def restated_members(x, spec):
    """Steps 1 and 2.  x [N,4,S,S] (``make_input``'s) -> the members' inputs [N,4,S_s,S_s], in member order."""
    S, out = x.shape[2], []
    for s, Ss, _, mirrored in member_table(spec, S):
        xs = x if Ss == S else R.resize_bilinear_tf(x, Ss, Ss, True)
        out.append(torch.flip(xs, [3]) if mirrored else xs)
    return out


def restated_member_logits(w, x, spec, nm):
    """Steps 3 and 4: every member's logits [N,2,L,L] (a mirrored member's: not yet reversed)."""
    out = []
    with torch.no_grad():
        for xm, (_, _, L, _) in zip(restated_members(x, spec), member_table(spec, x.shape[2])):
            lg = R.deeplab_logits(w, xm, nm)
            out.append(lg if lg.shape[2] == L else R.resize_bilinear_tf(lg, L, L, True))
    return out


def restated_merge(member_logits, spec, S=R.INPUT_SIZE):
    """Steps 5 to 7.  The members' L x L logits [N,2,L,L] -> (prob float32 [N,S,S], cls uint8 [N,S,S])."""
    table = member_table(spec, S)
    assert len(table) == len(member_logits)
    p0 = p1 = None
    for lg, (_, _, _, mirrored) in zip(member_logits, table):
        lg = lg.to(torch.float32)
        sm = torch.softmax(R.resize_bilinear_tf(torch.flip(lg, [3]) if mirrored else lg, S, S, False), dim=1)
        p0 = sm[:, 0] if p0 is None else p0 + sm[:, 0]
        p1 = sm[:, 1] if p1 is None else p1 + sm[:, 1]
    m = np.float32(len(table))
    P0, P1 = p0 / m, p1 / m
    return P1, (P1 > P0).to(torch.uint8)


def uncrop(prob, cls, crop, h, w):
    """Step 8 for ONE box (the second half of the oracle's ``output_layer``): prob [S,S], cls [S,S] -> (mask uint8 [h,w], posterior [h,w])."""
    y0, x0, y1, x1 = crop
    hc, wc = y1 - y0, x1 - x0
    mask = torch.zeros((h, w), dtype=torch.uint8)
    post = torch.zeros((h, w), dtype=torch.float32)
    if hc > 0 and wc > 0:
        mask[y0:y1, x0:x1] = R.resize_nearest_tf(cls[None, None].to(torch.float32), hc, wc)[0, 0].to(torch.uint8)
        post[y0:y1, x0:x1] = R.resize_bilinear_tf(prob[None, None], hc, wc, False)[0, 0]
    return mask.numpy(), post.numpy()


def restated_refine(w, img, box, spec, nm):
    """One box of one frame under ``spec`` -> (mask uint8 [h,w], posterior float32 [h,w], conf_score)."""
    h, wd = img.shape[:2]
    x, crop = R.make_input(img, box)
    prob, cls = restated_merge(restated_member_logits(w, x, spec, nm), spec, x.shape[2])
    mask, post = uncrop(prob[0], cls[0], crop, h, wd)
    return mask, post, R.conf_score(mask, post)
