"""Without a GPU: the checks of tests/conv_exact_device.py do assert.  Every exact conv suite relies on them to notice a word written
where none belongs; here each is handed a tiny host buffer tampered with in one word and has to raise an AssertionError that names
the case, and to pass the buffer as it was."""
import pytest
import torch

import conv_bf16_cases
import conv_f32_cases
import conv_wino_cases
from conv_exact_device import (SENTINEL, bits, check_unchanged, check_untouched, check_workspace, difference, extract_window,
                               input_buffer, sentinel_bits, windowed)

CASE = "the-case"
OFF, C, PS = 2, 3, 8                         # a window of 3 channels from channel 2 of 8-float pixels


def _out():
    """A 1 x 2 x 2 x 8 output buffer: sentinels around the window, values (with a NaN, which a written window may hold) inside."""
    values = torch.arange(12.0).view(1, 2, 2, C)
    values[0, 1, 1, 2] = float("nan")
    return windowed(values, PS, OFF, SENTINEL), values


def _raises(fn, *args, **kw):
    with pytest.raises(AssertionError, match=CASE):
        fn(*args, **kw)


def test_output_window_is_extracted_and_every_word_around_it_is_checked():
    buf, values = _out()
    assert torch.equal(bits(extract_window(CASE, buf, OFF, C)), bits(values))
    for channel in (OFF - 1, 0, OFF + C, PS - 1):                              # left of the window, right of it, both ends of the pixel
        bad = buf.clone()
        bad[0, 1, 0, channel] = 1.0
        _raises(extract_window, CASE, bad, OFF, C)
    bad = buf.clone()
    bits(bad)[0, 0, 1, OFF + C] += 1                                           # one bit of a sentinel
    _raises(extract_window, CASE, bad, OFF, C)
    inside = buf.clone()
    inside[0, 0, 0, OFF] = SENTINEL                                            # the window may hold anything
    extract_window(CASE, inside, OFF, C)
    # a window of no channels: the whole buffer has to hold the fill (an output a launch was not given); int32 words as well
    words = torch.full((1, 2, 2, PS), sentinel_bits(), dtype=torch.int32)
    assert extract_window(CASE, words, 0, 0, fill=sentinel_bits()).numel() == 0
    words[0, 1, 1, 5] = 0
    _raises(extract_window, CASE, words, 0, 0, fill=sentinel_bits())


def test_input_comparison_is_on_bits():
    before = torch.tensor([1.0, -0.0, 0.0, float("nan"), SENTINEL]).view(1, 1, 1, 5)
    check_unchanged(CASE, "input buffer", before.clone(), before)              # NaN == NaN here: same bits
    changed = before.clone()
    changed[..., 0] = 1.0000001
    _raises(check_unchanged, CASE, "input buffer", changed, before)
    for word, to in ((1, 0.0), (2, -0.0)):                                     # -0 <-> +0: equal as floats
        flipped = before.clone()
        flipped[..., word] = to
        assert (flipped == before)[..., word].all()
        _raises(check_unchanged, CASE, "input buffer", flipped, before)
    payload = before.clone()
    bits(payload)[..., 3] ^= 1                                                 # still a NaN, another payload
    assert torch.isnan(payload[..., 3]).all()
    _raises(check_unchanged, CASE, "input buffer", payload, before)


def test_workspace_has_to_be_written_up_to_the_last_word_asked_for_and_no_further():
    words, guard = 6, 4
    ws = torch.full((words + guard,), float("nan"))
    ws[:words] = torch.arange(6.0)
    check_workspace(CASE, ws, words)
    for unwritten in (0, 3, words - 1):
        bad = ws.clone()
        bad[unwritten] = float("nan")
        _raises(check_workspace, CASE, bad, words)
    for written in (words, words + guard - 1):
        bad = ws.clone()
        bad[written] = 0.0
        _raises(check_workspace, CASE, bad, words)


def test_refused_launch_must_leave_the_output_buffer_alone():
    out = torch.full((1, 2, 2, PS), SENTINEL)
    check_untouched(CASE, out)
    for channel in (0, OFF, PS - 1):                                           # inside the window as well: nothing ran
        bad = out.clone()
        bad[0, 1, 1, channel] = 0.0
        _raises(check_untouched, CASE, bad)


def test_difference_reports_count_first_index_and_largest_difference():
    ref = torch.zeros((1, 2, 2, 3))
    got = ref.clone()
    got[0, 1, 0, 2], got[0, 1, 1, 0] = 0.5, -2.0
    assert difference(CASE, "launch", got, ref) == (CASE, "launch", 2, [0, 1, 0, 2], 2.0)


TABLES = [(t, c) for t in (conv_f32_cases, conv_bf16_cases, conv_wino_cases) for c in t.CASES + getattr(t, "DENSE", [])]


@pytest.mark.parametrize("table,case", TABLES, ids=[f"{t.__name__[5:-6]}-{c.id}" for t, c in TABLES])
def test_input_round_trips_through_its_window(table, case):
    """windowed() and the window extraction are inverse bit for bit; the pad channels of the window are zero, all else is sentinel."""
    x = table.inputs(case).x
    cp = table.cin_pad(case)
    buf, off = input_buffer(x, cp, case.win_in)
    assert buf.shape == (case.n, case.h, case.w, case.win_in[0] if case.win_in else cp) and off == (case.win_in[1] if case.win_in else 0)
    window = extract_window(case.id, buf, off, cp)                             # asserts the sentinels around it
    assert torch.equal(bits(window[..., :case.cin].permute(0, 3, 1, 2)), bits(x))
    assert torch.all(bits(window[..., case.cin:]) == 0)
    assert (bits(buf) == sentinel_bits()).sum().item() == buf.numel() - window.numel()
