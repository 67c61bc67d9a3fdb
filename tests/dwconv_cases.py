"""The case table of the depthwise 3x3 kernel tests: which shapes tests/test_gpu_dwconv.py runs, and which kernel instance of
premvos_dwconv3x3_f32's dispatcher each of them launches (premvos_dwconv3x3_variant, encoding in include/premvos_hip.h).  A plain
module without a GPU: tests/test_cpu_dwconv_cover.py reads it to prove that every instance the dispatcher can pick -- on a sweep of
shapes and on the production layers -- has a case here, and that every threshold of the rule has a case on each side."""
from collections import namedtuple

S8 = 0x200                                   # PREMVOS_ACT_SPLIT8_BF16, OR-ed into `act`
RELU = 1
TILE, ROW, PIXEL = 1, 2, 3                   # PREMVOS_DW_TILE / _ROW / _PIXEL
F32, S8_UNPAIRED, S8_PAIRED = 0, 1, 2        # PREMVOS_DW_STORE_*
FAMILY_NAMES = {TILE: "tile", ROW: "row", PIXEL: "pixel"}
STORE_NAMES = {F32: "f32", S8_UNPAIRED: "s8", S8_PAIRED: "s8-paired"}


def code(family, tw, tr, ahead, pre_relu, stride, store):
    """The encoding documented at premvos_dwconv3x3_variant in include/premvos_hip.h."""
    return family | tw << 2 | tr << 5 | int(ahead) << 9 | int(pre_relu) << 10 | stride << 11 | store << 13


def decode(v):
    return dict(family=v & 3, tw=v >> 2 & 7, tr=v >> 5 & 15, ahead=v >> 9 & 1, pre_relu=v >> 10 & 1, stride=v >> 11 & 3, store=v >> 13 & 3)


def describe(v):
    d = decode(v)
    name = FAMILY_NAMES.get(d["family"], "?")
    if d["family"] == TILE:
        name += f"{d['tr']}x{d['tw']}" + ("" if d["ahead"] else "-noahead")
    elif d["family"] == ROW:
        name += f"-s{d['stride']}"
    return f"{name}{'+prerelu' if d['pre_relu'] else ''}/{STORE_NAMES.get(d['store'], '?')}"


# kernel instance without PRE_RELU and store form (those two come from the case's own pre_relu / act and c)
T55, T48, T44, T44N = (TILE, 5, 5, 1, 1), (TILE, 4, 8, 1, 1), (TILE, 4, 4, 1, 1), (TILE, 4, 4, 0, 1)
ROW1, ROW2, PIX = (ROW, 4, 1, 0, 1), (ROW, 4, 1, 0, 2), (PIXEL, 1, 1, 0, 0)

# n, c, h, w: the input maps; pt, pl: zero rows / columns in front of the map (taps behind it read zeros too); act: RELU and / or S8
# -- an S8 case runs the plain store as well and compares the two; win_in / win_out: (pixel stride, first channel) of the channel
# window the map occupies in a wider buffer, None = a buffer of its own; ho, wo: None = the extent that pads both sides by pt / pl;
# launches: the kernel instance the dispatcher must report for it.
Case = namedtuple("Case", "id n c h w stride rate pt pl pre_relu act win_in win_out ho wo launches")


def _c(id, n, c, h, w, stride, rate, pt, pl, pre_relu, act, launches, win_in=None, win_out=None, ho=None, wo=None):
    return Case(id, n, c, h, w, stride, rate, pt, pl, pre_relu, act, win_in, win_out, ho, wo, launches)


CASES = [
    # ---- 5x5 tiles (the 25x25 maps of the middle / exit flow; the only instance behind the XCD block permutation)
    _c("t55-25x25x728-pre", 3, 728, 25, 25, 1, 1, 1, 1, 1, S8, T55, (736, 4), (744, 8)),       # 54 workgroups: not a multiple of 8
    _c("t55-25x25x728", 2, 728, 25, 25, 1, 1, 1, 1, 0, RELU, T55),
    _c("t55-25x25x1024", 3, 1024, 25, 25, 1, 1, 1, 1, 0, RELU | S8, T55, (1032, 8), (1040, 16)),
    _c("t55-25x25x1024-pre", 1, 1024, 25, 25, 1, 1, 1, 1, 1, 0, T55),
    _c("t55-10x15x20", 7, 20, 10, 15, 1, 1, 1, 1, 0, S8, T55, (28, 4), (24, 0)),
    _c("t55-50x10x36-pre-nopad", 2, 36, 50, 10, 1, 1, 0, 0, 1, RELU | S8, T55, (40, 0), (44, 4), 50, 10),
    _c("t55-50x50x8", 1, 8, 50, 50, 1, 1, 1, 1, 0, 0, T55),
    # ---- 8x4 tiles (the wide entry-flow / decoder maps from 256 K threads upwards)
    _c("t48-193x193x64-pre", 16, 64, 193, 193, 1, 1, 1, 1, 1, S8, T48, (72, 8), (72, 0)),
    _c("t48-97x97x728", 5, 728, 97, 97, 1, 1, 1, 1, 0, RELU | S8, T48, (736, 8), (736, 0)),
    _c("t48-9x9x2044", 86, 2044, 9, 9, 1, 1, 1, 1, 0, S8, T48, (2052, 4), (2056, 8)),
    _c("t48-9x12x2044-pre", 90, 2044, 9, 12, 1, 1, 1, 1, 1, RELU | S8, T48),
    _c("t48-9x9x2048-n86", 86, 2048, 9, 9, 1, 1, 1, 1, 0, 0, T48),
    # ---- 4x4 tiles, dilation 1 ... 4 (a row loaded ahead)
    _c("t44-9x9x2048-n85", 85, 2048, 9, 9, 1, 1, 1, 1, 0, 0, T44),
    _c("t44-33x36x128-pre", 2, 128, 33, 36, 1, 1, 1, 1, 1, S8, T44, (136, 4), (144, 8)),
    _c("t44-20x23x20", 2, 20, 20, 23, 1, 1, 1, 1, 0, RELU | S8, T44, (24, 4), (28, 4)),
    _c("t44-31x34x12-r3-pre", 1, 12, 31, 34, 1, 3, 3, 3, 1, RELU | S8, T44, (20, 8), (16, 0)),
    _c("t44-25x25x2048-r2", 2, 2048, 25, 25, 1, 2, 2, 2, 0, RELU | S8, T44, (2056, 4), (2064, 8)),
    _c("t44-17x19x30-pre", 2, 30, 17, 19, 1, 1, 1, 1, 1, S8, T44, (40, 4), (40, 8)),            # c % 4 != 0
    _c("t44-13x14x8-r4", 1, 8, 13, 14, 1, 4, 4, 4, 0, 0, T44),
    _c("t44-55x55x8", 1, 8, 55, 55, 1, 1, 1, 1, 0, 0, T44),
    _c("t44-8x8x8", 1, 8, 8, 8, 1, 1, 1, 1, 0, 0, T44),
    _c("t44-23x29x16-nopad", 2, 16, 23, 29, 1, 1, 0, 0, 0, RELU, T44, (24, 4), (24, 8), 23, 29),   # ho, wo beyond the valid 21 x 27
    _c("t44-11x11x8-r2-nopad", 1, 8, 11, 11, 1, 2, 0, 0, 1, 0, T44),                             # valid extent 7 x 7
    # ---- 4x4 tiles on wide atrous layers, dilation >= 5 (no row in flight; masked-off taps hold arbitrary registers)
    _c("t44n-25x25x2048-r6", 2, 2048, 25, 25, 1, 6, 6, 6, 0, RELU | S8, T44N, (2052, 4), (2056, 8)),
    _c("t44n-25x25x2048-r12", 1, 2048, 25, 25, 1, 12, 12, 12, 0, RELU, T44N),
    _c("t44n-25x28x32-r12-pre", 1, 32, 25, 28, 1, 12, 12, 12, 1, S8, T44N),
    _c("t44n-19x17x12-r5", 2, 12, 19, 17, 1, 5, 5, 5, 0, S8, T44N, (16, 4), (24, 8)),
    _c("t44n-16x18x4-r6-pre", 1, 4, 16, 18, 1, 6, 6, 6, 1, RELU | S8, T44N),
    _c("t44n-13x14x8-r5", 1, 8, 13, 14, 1, 5, 5, 5, 0, 0, T44N),
    _c("t44n-13x13x8-r6", 1, 8, 13, 13, 1, 6, 6, 6, 0, 0, T44N),
    # ---- row kernel, stride 2 (the last depthwise conv of every strided entry / exit block)
    _c("row2-193to97x128-pre", 2, 128, 193, 193, 2, 1, 1, 1, 1, S8, ROW2, (136, 8), (136, 0)),
    _c("row2-193to97x64", 1, 64, 193, 193, 2, 1, 1, 1, 0, RELU, ROW2),
    _c("row2-49to25x728-pre", 2, 728, 49, 49, 2, 1, 1, 1, 1, 0, ROW2, (732, 4), (732, 0)),
    _c("row2-49to25x20", 3, 20, 49, 49, 2, 1, 1, 1, 0, S8, ROW2),
    _c("row2-26x31x12-pre-nopad", 1, 12, 26, 31, 2, 1, 0, 0, 1, RELU | S8, ROW2, (16, 0), (20, 4), 13, 16),
    _c("row2-34x37x256", 1, 256, 34, 37, 2, 1, 1, 1, 0, S8, ROW2),
    # ---- row kernel, stride 1 (maps under 8 rows)
    _c("row1-6x25x256-pre", 2, 256, 6, 25, 1, 1, 1, 1, 1, S8, ROW1, (264, 4), (272, 8)),
    _c("row1-1x8x8", 3, 8, 1, 8, 1, 1, 1, 1, 0, RELU | S8, ROW1),
    _c("row1-7x9x12", 2, 12, 7, 9, 1, 1, 1, 1, 0, S8, ROW1, (20, 4), (16, 4)),
    _c("row1-5x30x20-pre-nopad", 1, 20, 5, 30, 1, 1, 0, 0, 1, S8, ROW1, None, None, 5, 30),    # valid extent 3 x 28
    _c("row1-7x8x8", 1, 8, 7, 8, 1, 1, 1, 1, 0, 0, ROW1),
    # ---- per-pixel kernel (everything else: ASPP rate 18 on 25x25, maps under 8 columns, stride 3, strided atrous)
    _c("pix-25x25x2048-r18", 2, 2048, 25, 25, 1, 18, 18, 18, 0, RELU | S8, PIX, (2056, 8), (2056, 0)),
    _c("pix-1x1x16-pre", 2, 16, 1, 1, 1, 1, 1, 1, 1, S8, PIX),
    _c("pix-5x7x12-s3", 3, 12, 5, 7, 3, 1, 1, 1, 0, S8, PIX, (16, 4), (20, 8)),
    _c("pix-4x5x4-r2-pre", 1, 4, 4, 5, 1, 2, 2, 2, 1, RELU | S8, PIX),
    _c("pix-12x13x8-r6", 1, 8, 12, 13, 1, 6, 6, 6, 0, 0, PIX),
    _c("pix-7x7x8", 1, 8, 7, 7, 1, 1, 1, 1, 0, 0, PIX),
    _c("pix-11x11x8-s2-r2", 1, 8, 11, 11, 2, 2, 2, 2, 0, RELU, PIX),
    _c("pix-1x5x30-pre", 2, 30, 1, 5, 1, 1, 1, 1, 1, RELU, PIX, (36, 4), (40, 4)),
]
BY_ID = {c.id: c for c in CASES}

# every boundary of the dispatch rule: (what, the case on one side, the case on the other)
THRESHOLDS = [
    ("extent 8 against 7 at dilation 1", "t44-8x8x8", "row1-7x8x8"),
    ("ceil(extent / dilation) 3 against 2", "t44n-13x13x8-r6", "pix-12x13x8-r6"),
    ("wo 8 against 7 for the row kernel", "row1-7x8x8", "pix-7x7x8"),
    ("256 * 1024 threads", "t48-9x9x2048-n86", "t44-9x9x2048-n85"),
    ("ho <= 50 on extents that are multiples of 5", "t55-50x50x8", "t44-55x55x8"),
    ("dilation 4 against 5", "t44-13x14x8-r4", "t44n-13x14x8-r5"),
]


def c_pad(case):
    return (case.c + 3) // 4 * 4


def out_extent(case):
    ho = (case.h + 2 * case.pt - 2 * case.rate - 1) // case.stride + 1 if case.ho is None else case.ho
    wo = (case.w + 2 * case.pl - 2 * case.rate - 1) // case.stride + 1 if case.wo is None else case.wo
    return ho, wo


def store_form(case, act):
    return F32 if not act & S8 else S8_PAIRED if c_pad(case) // 4 % 2 == 0 else S8_UNPAIRED


def expected_code(case, act=None):
    """The code premvos_dwconv3x3_variant must return for the case run with ``act`` (default: the case's own)."""
    family, tw, tr, ahead, stride = case.launches
    return code(family, tw, tr, ahead, case.pre_relu, stride, store_form(case, case.act if act is None else act))


def launched_codes(case):
    """An S8 case runs twice: the plain store, which is its yardstick, and the S8 store."""
    return {expected_code(case, case.act & ~S8), expected_code(case)}


def query(lib, case, act=None, n=None):
    ho, wo = out_extent(case)
    return lib.premvos_dwconv3x3_variant(case.n if n is None else n, case.h, case.w, c_pad(case), ho, wo, case.stride, case.rate,
                                         case.pre_relu, case.act if act is None else act)


if __name__ == "__main__":                   # python tests/dwconv_cases.py: per variant code, the cases that launch it
    by_code = {}
    for case in CASES:
        for v in launched_codes(case):
            by_code.setdefault(v, []).append(case.id)
    for v in sorted(by_code, key=lambda v: (v & 3, describe(v))):
        print(f"{v:6d}  {describe(v):34s} {', '.join(by_code[v])}")
