"""Generates tests/golden/prewarp_neg_ref.npz / prewarp_neg_host_refs.json by IMPORTING AND EXECUTING MergeTrack/oldmerge.py (unmodified)
with its module switch ``use_ff_negative_props = True`` (oldmerge.py:43): ``do_video`` on two tiny videos of 40 x 56, under the shims
of tools/make_golden_prewarp.py (imported from there: the COCO RLE codec, the cv2.remap gather, the numpy stand-in that keeps what
np.argsort was handed).  Nothing of this package is imported.  tests/golden/prewarp_ref.npz is not touched.

Recorded per video: the negatives ``get_negative_ff_props`` returned (frame-0 proposal indices, in its order), per frame the five
planes, the array handed to np.argsort (oldmerge.py:176), the selections (the segmentations handed to decode, :177), the PNG arrays,
and ``eval_video``'s scores.

What the videos contain (asserted here; otherwise the next seed is tried):
  * "alpha": 3 objects, one of them annotated late (frame 2); "beta": 1 object;
  * frame-0 proposals that overlap an annotated object, that overlap one another (the lower-scored is refused), and disjoint ones;
  * two disjoint proposals of EQUAL score (taken in file order), and a proposal with an empty mask (taken);
  * a look-alike distractor: an unannotated ellipse whose embedding resembles object 1's; in frame ``EVENT`` its proposal is strong and
    the object's own are weak.  With the switch the distractor's own track keeps that column, without it object 1 takes it: the PNGs
    of the two runs must differ in at least one frame, and the negative must win a column that an object wins in the run without.

The margin condition of tools/make_golden_prewarp.py, kept (1e-6 >= the 1e-9 asked for): in every frame the first and second maximum of
every weighted column, and of every snapped row that something snapped to, differ by >= 1e-6; two selections whose masks overlap have
scores >= 1e-6 apart -- except rows that nothing snapped to: they hold exact zeros, choose column 0 and tie exactly, by construction
(np.argsort on <= 16 values is an insertion sort: the higher index paints last, the package's rule).  Data only.
Usage: python tools/make_golden_prewarp_neg.py <PReMVOS checkout>"""
import json
import os
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_golden_prewarp as G                                   # noqa: E402  (reads the checkout's path from sys.argv, runs nothing)

H, W, EMB, MARGIN, GOLD = G.H, G.W, G.EMB, G.MARGIN, G.GOLD
P, EVENT = 9, 3
J_DIS, J_RIVAL, J_A, J_B, J_EMPTY = 4, 5, 6, 7, 8                 # the distractor, one overlapping it, two of equal score, the empty mask


def run_reference(O, dirs, name, frames, switch):
    """do_video under the recorders -> (negatives, planes per frame, argsort inputs, decoded tags, eval scores, PNG arrays)"""
    O.to_do, O.image_dir, O.proposal_dir, O.ff_dir, O.gt_dir = "DAVIS", dirs["images"], dirs["props"], dirs["ff"], dirs["gt"]
    O.ensemble_output_dir = dirs["out_on"] if switch else dirs["out_off"]
    rec, planes_log, decoded, negs = G.Recorder(), [], [], []
    orig = (O.calculate_old_merge_scores, O.decode, O.np, O.get_negative_ff_props, O.use_ff_negative_props)

    def rec_scores(*a):
        planes = orig[0](*a)
        planes_log.append(np.array(planes))
        return planes

    def rec_decode(seg):
        decoded.append(seg["_idx"])
        return orig[1](seg)

    def rec_negatives(*a):
        out = orig[3](*a)
        negs.extend(p["segmentation"]["_idx"] for p in out)
        return out
    O.calculate_old_merge_scores, O.decode, O.np, O.get_negative_ff_props, O.use_ff_negative_props = rec_scores, rec_decode, rec, rec_negatives, switch
    try:
        scores = O.do_video(os.path.join(dirs["images"], name) + "/", 0)
    finally:
        O.calculate_old_merge_scores, O.decode, O.np, O.get_negative_ff_props, O.use_ff_negative_props = orig
    pngs = np.array([np.array(Image.open(os.path.join(O.ensemble_output_dir, "0", name, f"{t:05d}.png"))) for t in range(frames)])
    return negs, planes_log, np.array(rec.best), decoded, np.asarray(scores, np.float64), pngs


def build(seed, O, MF):
    rng = np.random.default_rng(seed)
    arrays, g = {}, {"seed": seed, "h": H, "w": W, "videos": {}, "event_frame": EVENT}
    g["weights"], g["normalised_weights"] = O.weights.tolist(), O.normalised_weights.tolist()
    margins = {"column": np.inf, "row": np.inf, "paint": np.inf}
    units = rng.integers(-8, 9, (8, EMB)).astype(np.float64) / 8.0

    def need(kind, value):
        margins[kind] = min(margins[kind], value)
        if value < MARGIN:
            raise G.TooClose(f"{kind}: {value}")

    def emb(i, noise):
        return np.round((units[i] + noise * rng.standard_normal(EMB)) * 64) / 64

    # (objects, velocities, start frames, the distractor's ellipse, the two equal-score clutter ellipses)
    for name, frames, objs, vel, starts, dis, clut in (
            ("alpha", 5, [(8, 10, 5, 6), (20, 40, 6, 7), (32, 14, 5, 8)], [(0, 3), (0, -3), (0, 2)], [0, 0, 2], (7, 38, 4, 5), ((35, 48, 3, 4), (35, 36, 3, 4))),
            ("beta", 5, [(20, 16, 7, 9)], [(0, 4)], [0], (34, 26, 4, 5), ((5, 8, 3, 4), (5, 46, 3, 4)))):
        n_obj = len(objs)
        bands = ((0, 14), (14, 27), (27, H)) if n_obj > 1 else ((0, H),)
        flow = np.zeros((frames - 1, H, W, 2), np.float32)
        for t in range(frames - 1):
            for (r0, r1), (dy, dx) in zip(bands, vel):
                flow[t, r0:r1] = (dx, dy)
        obj_emb = [emb(i, 0.05) for i in range(n_obj)]
        gt = np.zeros((frames, H, W), np.uint8)
        vid = {"frames": frames, "objects": [{"id": i + 1, "start": s} for i, s in enumerate(starts)]}
        p_mask, p_fwd = np.zeros((frames, P, H, W), np.uint8), np.zeros((frames, P, H, W), np.uint8)
        p_score, p_emb = np.zeros((frames, P)), np.zeros((frames, P, EMB))
        a_mask, a_fwd = np.zeros((n_obj, H, W), np.uint8), np.zeros((n_obj, H, W), np.uint8)
        equal_score = round(float(rng.uniform(0.4, 0.9)), 2)

        def fwd_of(m, t):
            return MF.warp_flow(m, flow[t].copy()) if t < frames - 1 else np.zeros((H, W), np.uint8)
        with tempfile.TemporaryDirectory() as td:
            dirs = {k: os.path.join(td, k) + "/" for k in ("images", "props", "ff", "gt", "out_on", "out_off")}
            for d in dirs.values():
                os.makedirs(os.path.join(d, name))
            for t in range(frames):
                Image.fromarray(np.full((H, W, 3), 90 + t, np.uint8)).save(os.path.join(dirs["images"], name, f"{t:05d}.jpg"))
                pos = [(cy + t * dy, cx + t * dx, ry, rx) for (cy, cx, ry, rx), (dy, dx) in zip(objs, vel)]
                for i, o in enumerate(pos):
                    gt[t][G.ellipse(*o) > 0] = i + 1
                im = Image.frombytes("P", (W, H), gt[t].tobytes())
                im.putpalette([0, 0, 0, 128, 0, 0] + [0] * (3 * 254))
                im.save(os.path.join(dirs["gt"], name, f"{t:05d}.png"))
                dpos = (dis[0] + t * vel[0][0], dis[1] + t * vel[0][1], dis[2], dis[3])      # the distractor rides on object 1's flow band
                props = []
                for j in range(P):
                    score = round(float(rng.uniform(0.3, 0.99)), 2)
                    if j < J_DIS:                                                   # the objects' own proposals
                        i = j % n_obj
                        if starts[i] > t:
                            i = j % 2
                        cy, cx, ry, rx = pos[i]
                        m = G.ellipse(cy + rng.integers(-2, 3), cx + rng.integers(-3, 4), ry + rng.integers(-1, 2), rx + rng.integers(-1, 3))
                        e = emb(i, 0.15) if j < n_obj else emb(i, 0.45)
                        if t == EVENT and i == 0:                                   # the event: object 1's own proposals are weak ...
                            score, e = round(float(rng.uniform(0.30, 0.36)), 2), emb(i, 0.6)
                    elif j == J_DIS:
                        m, e = G.ellipse(*dpos), emb(0, 0.08)                       # a look-alike of object 1
                        score = 0.99 if t == EVENT else round(float(rng.uniform(0.7, 0.9)), 2)        # ... and the distractor's is strong
                    elif j == J_RIVAL:                                              # overlaps the distractor, scores below it
                        m, e = G.ellipse(dpos[0] + 1, dpos[1] + 3, dpos[2], dpos[3]), emb(5, 0.4)
                        score = round(float(rng.uniform(0.3, 0.6)), 2)
                    elif j in (J_A, J_B):                                           # disjoint from everything; equal scores in frame 0
                        m, e = G.ellipse(*clut[j - J_A]), emb(6 + j - J_A, 0.3)
                        score = equal_score if t == 0 else score
                    else:
                        m, e = np.zeros((H, W), np.uint8), emb(4, 0.4)              # the empty mask
                    p = {"score": score, "segmentation": G.seg_str(m, j), "forward_segmentation": G.seg_str(fwd_of(m, t)), "ReID": e.tolist()}
                    if name == "alpha" and t == 1 and j == 3:
                        del p["ReID"]                                               # a proposal without 'ReID'
                        e = np.inf * np.ones(EMB)
                    p_mask[t, j], p_fwd[t, j], p_score[t, j], p_emb[t, j] = m, G.decode(p["forward_segmentation"]), p["score"], e
                    props.append(p)
                with open(os.path.join(dirs["props"], name, f"{t:05d}.json"), "w") as f:
                    json.dump(props, f)
                ff = []
                for i in range(n_obj):
                    if starts[i] == t:
                        m = (gt[t] == i + 1).astype(np.uint8)
                        a_mask[i], a_fwd[i] = m, fwd_of(m, t)
                        ff.append({"id": i + 1, "score": 1.0, "segmentation": G.seg_str(m, -(i + 1)), "forward_segmentation": G.seg_str(a_fwd[i]),
                                   "ReID": obj_emb[i].tolist()})
                if ff:
                    with open(os.path.join(dirs["ff"], name, f"{t:05d}.json"), "w") as f:
                        json.dump(ff, f)
            negs, planes_log, best, decoded, vid_scores, pngs = run_reference(O, dirs, name, frames, True)
            negs_off, _, _, decoded_off, _, pngs_off = run_reference(O, dirs, name, frames, False)
        # ---- what the fixture must show
        assert negs_off == []
        ann0 = [a_mask[i] for i in range(n_obj) if starts[i] == 0]
        touches = lambda j, others: any((p_mask[0, j] & o).any() for o in others)                 # noqa: E731
        if not (J_DIS in negs and J_RIVAL not in negs and J_EMPTY in negs and J_A in negs and J_B in negs and negs.index(J_A) < negs.index(J_B)):
            raise G.TooClose(f"negatives {negs}: the distractor, the two equal scores in file order and the empty mask must be taken, the rival not")
        assert touches(J_RIVAL, [p_mask[0, J_DIS]]) and not touches(J_RIVAL, ann0) and all(touches(j, ann0) for j in range(J_DIS))
        assert p_score[0, J_A] == p_score[0, J_B] and not p_mask[0, J_EMPTY].any() and not any(j in negs for j in range(J_DIS))
        if not any((pngs[t] != pngs_off[t]).any() for t in range(frames)):
            raise G.TooClose("the PNGs with and without the switch are equal: the fixture would show nothing")
        T_ann, T = n_obj, n_obj + len(negs)
        assert len(planes_log) == frames and len(best) == frames and len(decoded) == frames * T and len(decoded_off) == frames * T_ann
        first = np.concatenate(([0], np.cumsum([sum(1 for s in starts if s == t) for t in range(frames)])))
        chosen = np.array(decoded, np.int64).reshape(frames, T)
        chosen_off = np.array(decoded_off, np.int64).reshape(frames, T_ann)
        k_dis = T_ann + negs.index(J_DIS)
        stolen = [t for t in range(1, frames) if chosen[t, k_dis] == J_DIS and (chosen_off[t] == J_DIS).any() and not (chosen[t, :T_ann] == J_DIS).any()]
        if not stolen:
            raise G.TooClose("the distractor's track takes no column away from a real object in a later frame")
        vid["stolen_frames"] = stolen
        for t in range(frames):
            for k in range(T):
                if chosen[t, k] < 0:                                              # the annotation itself: the column after the proposals
                    assert first[t] <= k < first[t + 1] and chosen[t, k] == -(k + 1)
                    chosen[t, k] = P + k - first[t]
        assert (chosen[:, T_ann:] < P).all()                                      # a negative is forced in no frame
        zero_rows = 0
        for t in range(frames):
            weighted = np.dot(O.normalised_weights, planes_log[t].transpose((1, 0, 2)))
            assert planes_log[t].shape == (5, T, P)
            arrays[f"v_{name}_planes_{t}"], arrays[f"v_{name}_weighted_{t}"] = planes_log[t], weighted
            for p in range(P):
                need("column", G.second_gap(weighted[:, p]))
            closest = np.argmax(weighted, axis=0)
            sel, zero = [], []
            for k in range(T):
                row = weighted[k] * (closest == k)
                ann_now = first[t] <= k < first[t + 1]
                zero.append(not row.any() and not ann_now)
                zero_rows += zero[-1]
                if row.any() and not ann_now:
                    need("row", G.second_gap(row))
                sel.append(a_mask[k] if ann_now else p_mask[t, chosen[t, k]])
            for a in range(T):
                for b in range(a + 1, T):
                    if (sel[a] & sel[b]).any() and not (zero[a] and zero[b] and best[t, a] == 0.0 == best[t, b]):
                        need("paint", abs(best[t, a] - best[t, b]))
        arrays.update({f"v_{name}_gt": gt, f"v_{name}_png": pngs, f"v_{name}_png_off": pngs_off, f"v_{name}_chosen": chosen, f"v_{name}_best": best,
                       f"v_{name}_mask": p_mask, f"v_{name}_fwd": p_fwd, f"v_{name}_score": p_score, f"v_{name}_emb": p_emb,
                       f"v_{name}_ann_mask": a_mask, f"v_{name}_ann_fwd": a_fwd, f"v_{name}_ann_emb": np.array(obj_emb),
                       f"v_{name}_eval": vid_scores, f"v_{name}_negatives": np.array(negs, np.int64), f"v_{name}_flow": flow})
        vid["zero_score_rows"], vid["negatives"] = int(zero_rows), [int(i) for i in negs]
        g["videos"][name] = vid
    g["min_margin_column"], g["min_margin_row"], g["min_margin_paint"] = margins["column"], margins["row"], margins["paint"]
    return arrays, g


def main():
    O, MF = G.install()
    seed = 1
    while True:
        try:
            arrays, g = build(seed, O, MF)
            break
        except G.TooClose as e:
            print(f"seed {seed}: {e}; trying the next seed")
            seed += 1
            if seed > 400:
                sys.exit("no seed up to 400 meets the conditions: look at the generator")
    packed = {k: (np.packbits(v, axis=-1) if v.dtype == np.uint8 and k.endswith(("_mask", "_fwd")) else v) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(GOLD, "prewarp_neg_ref.npz"), **packed)
    with open(os.path.join(GOLD, "prewarp_neg_host_refs.json"), "w") as f:
        json.dump(g, f, separators=(",", ":"))
    for fn in ("prewarp_neg_ref.npz", "prewarp_neg_host_refs.json"):
        print(fn, os.path.getsize(os.path.join(GOLD, fn)), "bytes")
    assert os.path.getsize(os.path.join(GOLD, "prewarp_neg_ref.npz")) < 100 * 1000
    print("seed", g["seed"], "min margins", g["min_margin_column"], g["min_margin_row"], g["min_margin_paint"])
    for name, v in g["videos"].items():
        print(name, "negatives", v["negatives"], "stolen in frames", v["stolen_frames"], "zero-score rows", v["zero_score_rows"], "eval", arrays[f"v_{name}_eval"])


if __name__ == "__main__":
    main()
