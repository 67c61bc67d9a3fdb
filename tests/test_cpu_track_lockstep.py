"""The host side of ``track --lockstep`` (no GPU): header / binding / document agreement of the four seats entries, their argument
checks (before any HIP call, so they run here), ``plan_lockstep`` and the command line."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("premvos_mask_overlap_seats_u8", 9, "track_ops.hip"), ("premvos_track_scores_seats_f64", 18, "track_ops.hip"),
           ("premvos_track_paint_seats_u8", 15, "track_ops.hip"), ("premvos_mask_warp_seats_u8", 10, "merge_ops.hip"))


def test_header_signatures_and_documents_name_the_entries():
    from premvos_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "premvos_hip.h")).read()
    declared = set(re.findall(r"\b(premvos_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert _lib.ABI_VERSION == 21 and lib.premvos_abi_version() == 21                           # additive: the version stays
    for name, nargs, src in ENTRIES:
        assert name in declared and len(_lib.SIGNATURES[name]) == nargs and hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr).group(1)
        assert decl.count(",") + 1 == nargs, name                                               # as many parameters as the binding passes
        assert f'extern "C" int {name}(' in open(os.path.join(ROOT, "premvos_amd", "csrc", src)).read()
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (name, doc)
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(declared)} entry points, ABI v21" in open(os.path.join(ROOT, doc)).read(), doc
    for cite in ("merge_functions.py:38-45", "merge_functions.py:38-76", "merge_functions.py:123-149", "merge_functions.py:209-217", "seats[V][4]"):
        assert cite in hdr
    assert open(os.path.join(ROOT, "premvos_amd", "csrc", "track_ops.hip")).readline() == "// hipcc-flags: -ffp-contract=off\n"


def _table(*rows):
    return np.ascontiguousarray(np.array(rows, np.int32).reshape(-1, 4))


def test_the_entries_refuse_bad_arguments_before_any_hip_call():
    from premvos_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.int64)
    one = buf.ctypes.data                                                                       # never dereferenced: every call is refused
    weights = np.ones(5, np.float64)                                                            # (named: the arrays outlive the calls)
    w5 = weights.ctypes.data
    good = _table((2, 3, 0, 2), (0, 0, 0, 0), (1, 0, 5, 0))
    zero_slots, late_slots = np.zeros(8, np.int32), np.array([3, 0, 0], np.int32)
    slots = zero_slots.ctypes.data

    def overlap(masks=one, S=10, hw=16, seats=good, V=3, inter=one):
        return lib.premvos_mask_overlap_seats_u8(masks, S, hw, None if seats is None else seats.ctypes.data, V, inter, one, one, None)

    def scores(seats=good, V=3, inter=one, fresh=one, weights=w5):
        return lib.premvos_track_scores_seats_f64(inter, one, one, one, one, one, fresh, fresh, None if seats is None else seats.ctypes.data, V,
                                                  weights, 1e-10, one, one, one, one, one, None)

    def paint(masks=one, S=10, seats=good, V=3, R=4, rslots=slots, refined=one):
        return lib.premvos_track_paint_seats_u8(masks, S, 4, 4, None if seats is None else seats.ctypes.data, V, one, one, one, one, one,
                                                refined, R, rslots, None)

    def warp(masks=one, n=2, fom=one, flows=one, V=2, out=one + 64):
        return lib.premvos_mask_warp_seats_u8(masks, n, 4, 4, fom, flows, V, out, 1, None)

    def refused(rc, word):
        assert rc == -1 and word in lib.premvos_last_error(), (rc, lib.premvos_last_error())

    for f in (overlap, paint):
        refused(f(masks=None), b"null")
        refused(f(seats=None), b"null")
        refused(f(S=0), b"bad dims")
        refused(f(seats=_table((2, 3, 9, 2))), b"beyond")                                       # candidates 9, 10 of a pool of 10
        refused(f(seats=_table((2, 3, 0, 8))), b"beyond")                                       # fresh 8, 9, 10
        refused(f(seats=_table((2, 3, 10, 0))), b"beyond")                                      # a slot >= S
        refused(f(seats=_table((2, 3, -1, 2))), b"negative")
        refused(f(seats=_table((2, 3, 0, -2))), b"negative")
    refused(overlap(inter=None), b"null")
    refused(paint(refined=None), b"null")
    refused(paint(rslots=None), b"null")
    refused(paint(rslots=late_slots.ctypes.data), b"refined slots")          # planes 3, 4 of 4
    refused(scores(inter=None), b"null")
    refused(scores(weights=None), b"null")
    refused(scores(fresh=None), b"null")                                                        # a seat has fresh rows
    for f in (overlap, scores, paint):
        refused(f(V=0), b"seats")
        refused(f(V=9), b"seats")
        refused(f(seats=_table((256, 0, 0, 0)), V=1), b"255")
        refused(f(seats=_table((3, 65533, 0, 0)), V=1), b"65535")
        refused(f(seats=_table((-1, 0, 0, 0)), V=1), b"negative")
        refused(f(seats=_table((1, -1, 0, 0)), V=1), b"negative")
    for kw, word in ((dict(masks=None), b"null"), (dict(fom=None), b"null"), (dict(flows=None), b"null"), (dict(out=None), b"null"),
                     (dict(V=0), b"seats"), (dict(V=9), b"seats"), (dict(n=0), b"bad dims"), (dict(out=one), b"in-place")):
        refused(warp(**kw), word)
    # empty seats only: nothing to do, nothing launched (the slots of an empty seat are not looked at)
    empty = _table((0, 7, -3, 99), (0, 0, 0, 0))
    assert overlap(seats=empty, V=2) == 0 and scores(seats=empty, V=2, fresh=None) == 0 and paint(seats=empty, V=2) == 0


def test_seat_table_offsets():
    from premvos_amd import track
    st = track.SeatTable([(1, 1, 4, 9), (0, 5, 0, 0), (5, 12, 10, 20)])
    assert st.V == 3 and st.P.tolist() == [2, 0, 17] and st.F.tolist() == [1, 0, 12]            # an empty seat's F does not count
    assert st.oT.tolist() == [0, 1, 1, 6] and st.oF.tolist() == [0, 1, 1, 13] and st.oP.tolist() == [0, 2, 2, 19]
    assert st.oTP.tolist() == [0, 2, 2, 87]
    assert st.rows.dtype == np.int32 and st.rows.flags["C_CONTIGUOUS"] and st.ptr == st.rows.ctypes.data


def test_plan_lockstep():
    from premvos_amd.track import plan_lockstep
    big, small = (480, 854), (120, 200)
    videos = [("dog", big), ("bear", big), ("kite", small), ("camel", big), ("ant", small), ("zebra", (1080, 1920))]
    plan = plan_lockstep(videos, 2)
    assert plan == [(small, ["ant", "kite"]), (big, ["bear", "camel", "dog"]), ((1080, 1920), ["zebra"])]     # classes by their first name
    assert plan_lockstep(list(reversed(videos)), 2) == plan == plan_lockstep(videos, 2)                        # the same plan again
    assert plan_lockstep(videos, 8) == plan                                                                     # fewer videos than seats
    assert plan_lockstep(videos[:2], 4) == [(big, ["bear", "dog"])]
    # one seat: today's order, one video after another whatever their sizes
    assert plan_lockstep(videos, 1) == [(s, [n]) for n, s in sorted(videos)]
    assert [n for _, names in plan_lockstep(videos, 1) for n in names] == sorted(n for n, _ in videos)
    assert plan_lockstep([], 4) == []


def test_lockstep_flag(capsys):
    from premvos_amd import stream, track
    for bad in ("0", "9", "-1", "two"):
        with pytest.raises(SystemExit) as e:
            track.main(["--root", "/nonexistent", "--lockstep", bad])
        assert e.value.code == 2
        assert "--lockstep" in capsys.readouterr().err
    assert track.main(["--root", "/nonexistent", "--lockstep", "8", "--check-only"]) == 2       # accepted; the inputs are what is missing
    with pytest.raises(SystemExit):
        track.main(["--help"])
    help_text = capsys.readouterr().out
    assert "--lockstep" in help_text and "merge.py:69-115" in help_text and "not the bytes" in " ".join(help_text.split())
    with pytest.raises(SystemExit) as e:                                                        # the streaming driver keeps its one-video tracker
        stream.parse_args(["--track", "--lockstep", "2"])
    assert e.value.code == 2 and "unrecognized arguments: --lockstep" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        stream.parse_args(["--help"])
    assert "--lockstep" not in capsys.readouterr().out
