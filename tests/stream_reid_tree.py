"""The synthetic PReMVOS tree of tests/test_gpu_plumbing.py (``_make_tree``: same frames, same reduced nets, same layout), restated
for the --reid tests with the foreground biases of its random-weight nets raised, so that there IS something to embed.

Why, and how the shifts were picked (on the CPU, with the oracles alone): oracle/proposal_oracle.py ``detect_one_image`` on the five
'bear' frames of the plumbing tree finds NO detection with either proposal net (0 + 0 on every frame: all class scores stay
below RESULT_SCORE_THRESH), so refined_proposals/ holds empty lists and a ReID test on that tree would check nothing -- whatever the
refinement net does.  With the foreground class bias of both proposal nets raised by PROPOSAL_SHIFT = 2.0 the oracle finds 9 ... 12
detections on each 'bear' frame it was run on (0, 1, 2) and 4 ... 7 on 'camel' (the general net's; the specific net's scores stay
below the threshold), scores 0.50 ... 0.97, at least three of them above 0.6 on every frame.
oracle/refinement_oracle.py ``deeplab_logits`` on those boxes, resized to the crop, gives fg - bg logit = +8.2 (median) with
min -3.5 / max +14.8, i.e. 99.3 ... 99.8 % of every crop is foreground with the UNCHANGED reduced refinement weights: their masks are
non-empty without help, REFINE_SHIFT = 0.  (The full-depth synthetic refinement weights are the ones that need +7.5:
tools/time_merge_ingest.object_like_refinement_weights.)"""
import json

import numpy as np
import torch

from oracle import proposal_oracle as PO
from oracle import pwc_oracle as O
from oracle import refinement_oracle as RO
from oracle import reid_oracle as QO

BLOCKS, MIDDLE = (1, 1, 2, 1), 1
REID_UNITS = [QO.UNITS[0], ("res3", 2, (64, 64), (3, 3), (2, 1)), ("res15", 3, (32, 64, 96), (1, 3, 1), (1, 2, 1))]
REID_NETWORK = {"conv0": {"class": "Conv", "n_features": 64, "activation": "linear"},
                "res0": {"class": "ResidualUnit2", "n_features": 128, "strides": [[2, 2], [1, 1]], "from": ["conv0"]},
                "res3": {"class": "ResidualUnit2", "n_features": 64, "strides": [[2, 2], [1, 1]], "from": ["res0"]},
                "res15": {"class": "ResidualUnit2", "n_convs": 3, "n_features": [32, 64, 96],
                          "filter_size": [[1, 1], [3, 3], [1, 1]], "strides": [[1, 1], [2, 2], [1, 1]], "from": ["res3"]},
                "conv1": {"class": "Conv", "n_features": 500, "batch_norm": True, "filter_size": [3, 3], "pool_size": [3, 3],
                          "from": ["res15"]},
                "fc1": {"class": "FullyConnected", "n_features": 500, "batch_norm": True, "from": ["conv1"]},
                "fc2": {"class": "FullyConnected", "n_features": 500, "batch_norm": True, "from": ["fc1"]},
                "outputTriplet": {"class": "FullyConnectedWithTripletLoss", "n_features": 128, "batch_norm": True,
                                  "activation": "linear", "from": ["fc2"]}}
PROPOSAL_SHIFT = 2.0    # added to fastrcnn/class/b[1] of both proposal nets
REFINE_SHIFT = 0.0      # added to logits/features/biases[1] of the refinement net
STREAM_ARGS = ["--flow_weights", "weights/pwc.pth.tar", "--general_weights", "weights/proposal_general_weights",
               "--specific_weights", "weights/specific.pt", "--refinement_weights", "weights/refinement_specific_weights"]


def refinement_weights():
    w = RO.synth_weights(0, MIDDLE)
    w["logits/features/biases"] = w["logits/features/biases"] + torch.tensor([0.0, REFINE_SHIFT])
    return w


def proposal_weights(seed):
    w = PO.synth_weights(seed, BLOCKS)
    w["fastrcnn/class/b"] = w["fastrcnn/class/b"] + torch.tensor([0.0, PROPOSAL_SHIFT])
    return w


def make_tree(root, h=120, w=200, t=5, videos=None):
    """``videos``: {name: frames}; default one clip 'bear' of ``t`` frames (its decoded frames are returned)."""
    from PIL import Image
    from premvos_amd import weights as W
    videos = videos or {"bear": t}
    frames = []
    for vi, (name, nt) in enumerate(videos.items()):
        seq_dir = root / "data" / "DAVIS" / "JPEGImages" / "480p" / name
        seq_dir.mkdir(parents=True)
        for i in range(nt):
            pair = O.synth_frame_pair(h, w + (-w) % 8, seed=40 + vi, shift=(1.5 * i, -0.5 * i))
            img = (pair[0, 3:, :, :w].permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()
            Image.fromarray(img).save(seq_dir / f"{i:05d}.jpg", quality=95)
            if vi == 0:
                frames.append(np.asarray(Image.open(seq_dir / f"{i:05d}.jpg").convert("RGB")))
    (root / "seq_to_run.txt").write_text("".join(f"data/DAVIS/JPEGImages/480p/{name}/\n" for name in videos))
    wd = root / "weights"
    wd.mkdir()
    torch.save({"state_dict": O.synth_state_dict(0)}, wd / "pwc.pth.tar")
    W.save_tf_checkpoint(str(wd / "proposal_general_weights"), W.proposal_weights_to_tf(proposal_weights(0)))
    torch.save(proposal_weights(1), wd / "specific.pt")
    W.save_tf_checkpoint(str(wd / "refinement_specific_weights"), W.refinement_weights_to_tf(refinement_weights()))
    # ReID: config under code/ReID_net/configs/ with a relative 'load' (the reference runs that stage from code/)
    W.save_tf_checkpoint(str(wd / "ReID_general_weights"), W.reid_weights_to_tf(QO.synth_weights(0, REID_UNITS)))
    cdir = root / "code" / "ReID_net" / "configs"
    cdir.mkdir(parents=True)
    (cdir / "run").write_text("# reduced ReID net for the plumbing test\n" + json.dumps(
        {"model": "Re-ID", "load": "../weights/ReID_general_weights", "input_size": [128, 128], "network": REID_NETWORK}))
    return frames


def reid_engine(root):
    """The stage driver's engine for the tree's config, its 'load' resolved from code/ as tools/run_stages.py does."""
    import os
    from premvos_amd.reid import driver as qd
    path = str(root / "code" / "ReID_net" / "configs" / "run")
    cfg = qd.Config(path)
    cfg._entries["load"] = os.path.normpath(os.path.join(str(root / "code"), cfg.str("load")))
    return qd.engine_from_config(cfg)
