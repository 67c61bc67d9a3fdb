"""premvos_mask_warp_pack_bits_u8 and `prewarp.VideoIngest` on the GPU.  The yardstick is the pair the pool was made with before --
premvos_mask_warp_seats_u8 (in groups of at most 8 flows) plus premvos_mask_pack_bits_u8 -- and `prewarp.pack_bits_host` for the
layout; every comparison is bit for bit and covers every mask of every frame."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (7, 9), (8, 8), (5, 13), (24, 32), (120, 200))       # tail word, 63, exactly 64, 65, a wave that straddles rows, the tree tests' size
# (masks per frame, flow of each frame, number of flows)
LAYOUTS = {"one frame": ([4], [0], 1),
           "an empty frame in the middle": ([3, 0, 2], [0, 1, 2], 3),
           "nine frames": ([2, 1, 3, 1, 1, 2, 1, 1, 2], list(range(9)), 9),
           "a frame without flow": ([2, 2, 2], [0, -1, 1], 2),
           "two frames share a flow": ([2, 2], [0, 0], 1)}
FLOWS = ("zero", "subpixel", "saturating")


def _masks(rng, n, h, w):
    """0/1 blobs; mask 0 all zero, mask 1 all one, mask 2 of bytes 0 / 255"""
    m = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[i, y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = 1
        m[i] ^= (rng.random((h, w)) < 0.08).astype(np.uint8)
    m[0] = 0
    m[1] = 1
    m[2] *= 255
    return m


def _flows(rng, kind, nf, h, w):
    if kind == "zero":
        return np.zeros((nf, h, w, 2), np.float32)
    f = rng.uniform(-3, 3, (nf, h, w, 2)).astype(np.float32)
    if kind == "saturating":                                           # beyond the int16 cell of the remap, both signs
        flat = f[0].reshape(-1)
        big = np.array([1e6, -1e6, 40000.5, -40000.5], np.float32)
        idx = rng.permutation(flat.size)[:max(4, flat.size // 6)]
        flat[idx] = big[np.arange(idx.size) % 4]
        flat[:min(4, flat.size)] = big[:min(4, flat.size)]
    return f


def _yardstick(masks, counts, fof, flows):
    from premvos_amd import mergetrack as mt, prewarp as pw
    n, h, w = masks.shape
    m = torch.from_numpy(masks).cuda()
    fl = torch.from_numpy(flows).cuda()
    fom = np.concatenate([np.full(c, f, np.int32) for c, f in zip(counts, fof)])
    fwd = torch.zeros_like(m)
    for g0 in range(0, flows.shape[0], pw.MAX_WARP_FLOWS):
        grp = np.where((fom >= g0) & (fom < g0 + pw.MAX_WARP_FLOWS), fom - g0, -1).astype(np.int32)
        mt.warp_masks_seats(m, torch.from_numpy(grp).cuda(), fl[g0:g0 + pw.MAX_WARP_FLOWS].contiguous(), out=fwd)
    rb = pw.row_bytes(h * w)
    cur_bits, fwd_bits = (torch.full((n, rb), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2))
    pw.pack_rows(m, cur_bits)
    pw.pack_rows(fwd, fwd_bits)
    return cur_bits.cpu().numpy(), fwd_bits.cpu().numpy(), fwd.cpu().numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_rows_equal_warp_seats_plus_pack_bits(h, w):
    from premvos_amd import prewarp as pw
    rng = np.random.default_rng(1000 * h + w)
    for name, (counts, fof, nf) in LAYOUTS.items():
        n = sum(counts)
        masks = _masks(rng, n, h, w)
        for kind in FLOWS:
            flows = _flows(rng, kind, nf, h, w)
            want_cur, want_fwd, fwd_bytes = _yardstick(masks, counts, fof, flows)
            cur, fwd = pw.warp_pack_rows(torch.from_numpy(masks).cuda(), counts, torch.from_numpy(flows).cuda(), flow_of_frame=fof)
            cur, fwd = cur.cpu().numpy(), fwd.cpu().numpy()
            what = (name, kind, h, w)
            assert cur.shape == fwd.shape == (n, pw.row_bytes(h * w)), what
            assert np.array_equal(want_cur, pw.pack_bits_host(masks)), what                  # the yardstick holds the layout
            assert np.array_equal(want_fwd, pw.pack_bits_host(fwd_bytes)), what
            assert np.array_equal(cur, want_cur), what
            assert np.array_equal(fwd, want_fwd), what
            assert cur[2].any() == bool(masks[2].any()) and not cur[0].any(), what           # bytes of 255 are set bits
            moved = np.concatenate([np.full(c, f >= 0) for c, f in zip(counts, fof)])
            assert not fwd[~moved].any(), what                                               # no flow: all-zero forward rows
            if kind == "zero":                                                               # the identity map: forward = the bytes that are 1
                assert np.array_equal(fwd, pw.pack_bits_host((masks == 1).astype(np.uint8)) * moved[:, None]), what
        if h * w >= 64:
            assert want_fwd.any(), name                                                      # the comparison is of something


def _video(rng, h, w):
    """a 6-frame video as ``upload()`` takes it ("mask" + "flow"), and the same as the streaming driver has it (rows, scores)"""
    P = [3, 2, 0, 4, 1, 3]
    frames, rows, scores = [], [], []
    for t, p in enumerate(P):
        m = np.zeros((p, h, w), np.uint8)
        for i in range(p):
            y0, x0 = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
            m[i, y0:y0 + int(rng.integers(4, 12)), x0:x0 + int(rng.integers(4, 14))] = 1
        e32 = rng.standard_normal((p, 128)).astype(np.float32)
        box = np.tile(np.array([1, 2, 5, 6], np.int32), (p, 1))
        sc = [float(x) for x in rng.uniform(0.3, 1.0, p)]
        emb = e32.astype(np.float64)
        if t == 3:
            box[2] = [4, 4, 0, 7]                                                            # a degenerate box: no "ReID" in the file -> all +inf
            emb[2] = np.inf
        fr = {"score": sc, "emb": emb, "mask": m, "ann": []}
        if t + 1 < len(P):
            fr["flow"] = rng.uniform(-2.5, 2.5, (h, w, 2)).astype(np.float32)
        frames.append(fr)
        rows.append(np.concatenate([e32, box.view(np.float32)], axis=1))
        scores.append(np.asarray(sc, np.float64))
    ann = np.zeros((h, w), np.uint8)
    ann[2:12, 3:15] = 1
    ann[10:20, 14:30] = 3
    for i in (1, 3):
        frames[0]["ann"].append({"id": i, "mask": (ann == i).astype(np.uint8), "reid": rng.standard_normal(128)})
    for i, obj in enumerate(frames[0]["ann"]):                                              # a proposal of every frame near each object
        for fr in frames:
            if len(fr["score"]) > i:
                fr["mask"][i] = obj["mask"]
                fr["emb"][i] = obj["reid"].astype(np.float32).astype(np.float64)
    for t, fr in enumerate(frames):
        rows[t][:, :128] = np.where(np.isinf(fr["emb"]), rows[t][:, :128], fr["emb"].astype(np.float32))
    return frames, P, rows, scores


def test_ingest_in_chunks_builds_the_pool_of_upload():
    from premvos_amd import prewarp as pw
    h, w = 24, 32
    frames, P, rows, scores = _video(np.random.default_rng(11), h, w)
    want = pw.upload(frames, h, w)
    ing = pw.VideoIngest(h, w)
    dev = want.dev
    ing.add_annotations(frames[0]["ann"], torch.from_numpy(frames[0]["flow"]).to(dev))
    t0 = 0
    for n in (2, 3, 1):
        ts = list(range(t0, t0 + n))
        masks = torch.from_numpy(np.concatenate([frames[t]["mask"] for t in ts])).to(dev)
        fl = [frames[t]["flow"] for t in ts if "flow" in frames[t]]
        ing.add_chunk(masks, [P[t] for t in ts], torch.from_numpy(np.stack(fl)).to(dev) if fl else None,
                      torch.from_numpy(np.concatenate([rows[t] for t in ts])).to(dev), torch.from_numpy(np.concatenate([scores[t] for t in ts])).to(dev))
        t0 += n
    got = ing.finish()
    assert got.tab.blocks.tolist() == want.tab.blocks.tolist() and got.ids == want.ids == [1, 3]
    assert got.pool.shape == want.pool.shape and torch.equal(got.pool, want.pool)
    assert want.pool[want.tab.fwd0:want.tab.fwd0 + want.tab.sumP].any() and want.pool[want.tab.annfwd0:].any()
    assert not want.pool[want.tab.fwd0 + int(want.tab.poff[5]):want.tab.fwd0 + want.tab.sumP].any()                # the last frame moves nowhere
    for name in ("score", "emb_p", "emb_t"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    row = int(want.tab.poff[3]) + 2
    assert torch.isinf(want.emb_p[row]).all() and torch.isfinite(want.emb_p[:row]).all() and torch.isfinite(want.emb_p[row + 1:]).all()
    got.prepare()
    c = got.chain(pw.normalised()[None])
    idmap, _ = got.paint(c["chosen"], c["best"])
    ref = pw.merge_video(frames, h, w)
    ref["ready"].synchronize()
    assert np.array_equal(idmap.cpu().numpy(), ref["idmap"].numpy())
    assert set(np.unique(ref["idmap"].numpy()[0])) == {0, 1, 3} and ref["idmap"].numpy()[-1].any()
