"""Test-time augmentation of the refinement net: which members a spec stands for.

The reference's DeepLab module runs the net on the crop at several scales, each optionally mirrored, and averages the members'
softmax probabilities (refinement_net/network/deeplab/model.py:84-160 predict_labels_multi_scale; the scale handling is
model.py:200-325).  A spec is a list of scales from DeepLab's set plus a flip flag; its text form is "0.75,1,1.25" or
"0.75,1,1.25+flip".  Host only: no GPU, no library.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)       # DeepLab's eval_scales
MAX_MEMBERS = 12                                 # PREMVOS_TTA_MAX_MEMBERS: six scales, each mirrored
INPUT_SIZE = 385


def scale_dimension(dim: int, scale: float) -> int:
    """model.py:184-197."""
    return int((float(dim) - 1.0) * scale + 1.0)


class TTA:
    """``scales`` in the order given (no repeats, each one of ``SCALES``), ``flip``: every scale also mirrored."""

    def __init__(self, scales: Sequence[float], flip: bool = False):
        scales = [float(s) for s in scales]
        if not scales:
            raise ValueError("a TTA spec needs at least one scale")
        if len(scales) * (2 if flip else 1) > MAX_MEMBERS:
            raise ValueError(f"{len(scales) * (2 if flip else 1)} members (at most {MAX_MEMBERS})")
        for i, s in enumerate(scales):
            if s not in SCALES:
                raise ValueError(f"unknown scale {s:g} (one of {', '.join(f'{x:g}' for x in SCALES)})")
            if s in scales[:i]:
                raise ValueError(f"scale {s:g} is listed twice")
        if not isinstance(flip, (bool, int)) or flip not in (0, 1):
            raise ValueError(f"flip is a bool, not {flip!r}")
        self.scales: Tuple[float, ...] = tuple(scales)
        self.flip = bool(flip)

    @property
    def plain(self) -> bool:
        """The single member (1.0, unmirrored): plain inference."""
        return self.scales == (1.0,) and not self.flip

    def members(self, size: int = INPUT_SIZE) -> List[Tuple[float, int, int, bool]]:
        """(scale, S_s, L, mirrored) in member order: per scale as listed the unmirrored crop, then (flip) the mirrored one.
        S_s = scale_dimension(size, scale): the member's input (model.py:272-277); L = scale_dimension(size, max(1, scale) / 4): the
        grid its logits are brought to (model.py:258-297)."""
        out = []
        for s in self.scales:
            for mirrored in ((False, True) if self.flip else (False,)):
                out.append((s, scale_dimension(size, s), scale_dimension(size, max(1.0, s) / 4.0), mirrored))
        return out

    def __str__(self) -> str:
        return ",".join(f"{s:g}" for s in self.scales) + ("+flip" if self.flip else "")

    def __repr__(self) -> str:
        return f"TTA({str(self)!r})"

    def __eq__(self, other) -> bool:
        return isinstance(other, TTA) and (self.scales, self.flip) == (other.scales, other.flip)

    def __hash__(self) -> int:
        return hash((self.scales, self.flip))

    def describe(self, size: int = INPUT_SIZE) -> str:
        """One line naming the members."""
        return "  ".join(f"{s:g}{'m' if mirrored else ''}@{ss}" for s, ss, _, mirrored in self.members(size))


def parse(text: str) -> TTA:
    """"0.75,1,1.25" / "0.75,1,1.25+flip" -> the spec; a ValueError names the offending token."""
    if not isinstance(text, str) or not text.strip():
        raise ValueError("an empty TTA spec (scales like 0.75,1,1.25, optionally followed by +flip)")
    body, plus, tail = text.strip().partition("+")
    if plus and tail.strip() != "flip":
        raise ValueError(f"unknown suffix {'+' + tail!r} (only +flip)")
    scales = []
    tokens = body.split(",")
    if len(tokens) * (2 if plus else 1) > MAX_MEMBERS:
        raise ValueError(f"{len(tokens) * (2 if plus else 1)} members in {text.strip()!r} (at most {MAX_MEMBERS})")
    for tok in tokens:
        try:
            s = float(tok)
        except ValueError:
            raise ValueError(f"not a scale: {tok.strip()!r} (one of {', '.join(f'{x:g}' for x in SCALES)})") from None
        if s not in SCALES:
            raise ValueError(f"unknown scale {tok.strip()!r} (one of {', '.join(f'{x:g}' for x in SCALES)})")
        if s in scales:
            raise ValueError(f"scale {tok.strip()!r} is listed twice")
        scales.append(s)
    return TTA(scales, bool(plus))


def resolve(spec: Union[None, str, TTA, Sequence[float]], flip: Optional[bool] = None) -> Optional[TTA]:
    """Whatever a caller holds -- None, the text form, a ``TTA``, a list of scales (with ``flip``) -- -> the spec, or None when it is
    off or stands for plain inference ("1")."""
    if spec is None:
        return None
    t = spec if isinstance(spec, TTA) else parse(spec) if isinstance(spec, str) else TTA(spec, bool(flip))
    return None if t.plain else t
