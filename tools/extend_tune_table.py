#!/usr/bin/env python
"""Adds to premvos_amd/tune_gfx950.json the conv signatures that the shipped table does not hold yet (a kernel option that changes
which filters a layer packs -- F(4x4,3x3) from 64 input channels, 32-channel outputs -- or a plan that runs a layer on another
tensor -- the RoI head's projected conv1 and its stride-1 shortcut -- changes the layer's signature): family and k-slices by the
closed-form rule (ops.rule_choice), the order-neutral knobs timed once, here, instead of at every plan build.  Existing entries are
not touched.  Shapes: the ones tools/make_tune_table.py covers for the stage (default: the flow net; --proposal: the proposal net).

    python tools/extend_tune_table.py [--proposal] [--with-1080p]
"""
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("PREMVOS_TUNE_CACHE", None)
import torch  # noqa: E402

from premvos_amd import ops, synth  # noqa: E402
from premvos_amd.flow.driver import FlowStage  # noqa: E402
from premvos_amd.proposal.driver import ProposalStage  # noqa: E402


def main():
    before = {json.dumps(k) for k, _ in json.load(open(ops.TUNE_TABLE))}
    proposal = "--proposal" in sys.argv
    w = synth.proposal_weights(0) if proposal else synth.pwc_state_dict(0)
    shapes = [(480, 854, b) for b in (16, 8, 1, 2, 4)] + ([(1080, 1920, 16)] if "--with-1080p" in sys.argv else [])
    for h, wd, b in shapes:
        fa, fb = synth.video_frames(b, h, wd, 0)
        if proposal:            # (the general and the specific net have the same signatures)
            st = ProposalStage(w, batch=b, rgb_input=True, use_graph=False)
            st.run(fa.cuda())
        else:
            st = FlowStage(w, batch=b, use_graph=False)
            st.run(fa.cuda(), fb.cuda())
        torch.cuda.synchronize()
        del st
        gc.collect()
        torch.cuda.empty_cache()
        print(f"{'proposal' if proposal else 'flow'} stage {h}x{wd} x {b}: {len(ops._TUNE_CACHE)} signatures", flush=True)
    ops.save_tune_cache(ops.TUNE_TABLE)
    table = json.load(open(ops.TUNE_TABLE))
    new = [(k, v) for k, v in table if json.dumps(k) not in before]
    for k, v in new:
        print("  +", k[:13], v)
    print(f"wrote {ops.TUNE_TABLE}: {len(table)} signatures ({len(new)} new)")


if __name__ == "__main__":
    main()
