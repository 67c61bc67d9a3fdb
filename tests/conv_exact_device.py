"""The device harness the exact conv tests share (tests/test_gpu_conv_{f32,bf16,f32_special,wino_exact,s8_exact}.py): a case's maps
inside channel windows of sentinel-filled buffers, a NaN-filled workspace of exactly the size the library asks for, and the checks
that a launch wrote its window and its workspace and nothing else.  The checks are plain functions on host tensors -- DeviceLayer
hands them copies -- and tests/test_cpu_conv_exact_harness.py holds them to their word without a GPU.  Everything compares bits."""
import ctypes

import torch
import torch.nn.functional as F

from conv_exact import nhwc, round_up

SENTINEL = 12345678.0                        # exactly representable; compared bit for bit
GUARD_WORDS = 64                             # NaN words behind the workspace a launch is handed


def ops():
    from premvos_amd import _lib, ops
    return _lib, _lib.load(), ops


def bits(t):
    return t.contiguous().view(torch.int32)


def sentinel_bits():
    return bits(torch.tensor([SENTINEL]))[0].item()


def tile_hint(tile):
    return (tile[0] << 16) | tile[1]


def difference(case_id, name, got, ref):
    """-> (case, launch, elements that differ, the first of them, largest difference)."""
    bad = got != ref
    return (case_id, name, int(bad.sum()), bad.nonzero()[0].tolist(), (got - ref).abs().max().item())


def shape_desc(table, case):
    """The shape fields of the descriptor of a case of the fp32 tables (what premvos_conv2d_workspace_bytes and ops._candidates read):
    no device pointers, no GPU."""
    from premvos_amd import _lib
    d = _lib.ConvDesc()
    d.n, d.h, d.w = case.n, case.h, case.w
    d.ho, d.wo = table.gemm_extent(case)
    d.cin, d.cin_pad, d.cout, d.cout_pad = case.cin, table.cin_pad(case), table.gemm_cout(case), table.cout_pad(case)
    d.in_ps = (case.win_in or (table.cin_pad(case), 0))[0]
    d.out_ps = (case.win_out or (round_up(case.cout, 4), 0))[0]
    d.kh = d.kw = 3 if case.deconv else case.k
    d.sh = d.sw = case.stride
    d.dh = d.dw = case.dil
    d.pt, d.pl = (1, 1) if case.deconv else case.pad[:2]
    d.k_pad = table.k_pad(case)
    d.precision = _lib.PRECISIONS["fp32"]
    d.out_mode, d.cout_ps = (_lib.OUT_PIXSHUF2, case.cout) if case.deconv else (_lib.OUT_NHWC, 0)
    return d


# ---- buffers and their checks, on the host ---------------------------------------------------------------------------------------------

def windowed(values_nhwc, pixel_stride, offset, fill):
    """NHWC values inside their channel window of a buffer of that pixel stride, of their dtype, otherwise holding ``fill``."""
    buf = torch.full(values_nhwc.shape[:-1] + (pixel_stride,), fill, dtype=values_nhwc.dtype)
    buf[..., offset:offset + values_nhwc.shape[-1]] = values_nhwc
    return buf


def input_buffer(x_nchw, cin_pad, win):
    """The input map inside its window (pixel stride, first channel) of a sentinel-filled buffer; the pad channels of the window are
    zero and meet zero weights.  None: a buffer of its own.  -> (buffer, first channel)."""
    ps, off = win or (cin_pad, 0)
    return windowed(F.pad(nhwc(x_nchw), (0, cin_pad - x_nchw.shape[1])), ps, off, SENTINEL), off


def check_unchanged(label, what, now, before):
    assert torch.equal(bits(now), bits(before)), f"{label}: the {what} was written"


def extract_window(label, buf, offset, channels, fill=SENTINEL):
    """-> the channel window of an NHWC buffer, after asserting that every word around it still holds ``fill``."""
    words = bits(buf)
    outside = torch.cat([words[..., :offset], words[..., offset + channels:]], -1)
    assert torch.all(outside == bits(torch.tensor([fill], dtype=buf.dtype))[0].item()), f"{label}: channels outside the window were written"
    return buf[..., offset:offset + channels].contiguous()


def check_untouched(label, buf):
    assert torch.all(bits(buf) == sentinel_bits()), f"{label}: a refused launch wrote"


def check_workspace(label, ws, words):
    """Every one of the ``words`` the library asked for was written, none of the NaN words behind them."""
    nan = torch.isnan(ws)
    assert not nan[:words].any() and nan[words:].all(), f"{label}: the workspace was not written as the query says"


# ---- a case on the device --------------------------------------------------------------------------------------------------------------

class DeviceLayer:
    """One case on the device: the input inside its channel window of a sentinel-filled buffer, the output window, the residual, packed
    weights, descriptor.  A subclass names its case table (cin_pad, out_extent, SLOPE), packs the weights, asserts the descriptor fields
    its table counts on, and has a `run` of its own."""
    table = None
    RES_WINDOWED = False                     # the residual lies in a sentinel-filled window (case.win_res), not in a buffer of its own

    def pack(self, ops, data):
        raise NotImplementedError

    def check_desc(self, _lib, ops, d):
        pass

    def __init__(self, case, data, stride=None, out_hw=None):
        _lib, lib, ops_ = ops()
        self.case, self.ops, self.ws = case, ops_, None
        deconv = getattr(case, "deconv", False)
        stride = stride or getattr(case, "stride", 1)
        self.before, off = input_buffer(data.x, self.table.cin_pad(case), case.win_in)
        self.xin = self.before.cuda()
        ho, wo = out_hw or self.table.out_extent(case)
        out_ps, self.off = case.win_out or (round_up(case.cout, 4), 0)
        self.out = torch.empty((case.n, ho, wo, out_ps), device="cuda")
        self.pk = self.pack(ops_, data)
        self.res = None
        if data.res is not None and self.RES_WINDOWED:
            res_ps, res_off = case.win_res or (round_up(case.cout, 4), 0)
            self.res = ops_.NHWC(windowed(nhwc(data.res), res_ps, res_off, SENTINEL).cuda(), c=case.cout, coff=res_off)
        elif data.res is not None:
            self.res = ops_.NHWC.alloc(case.n, ho, wo, case.cout)
            self.res.buf[..., :case.cout] = nhwc(data.res).cuda()
        act = {"none": ops_.ACT_NONE, "relu": ops_.ACT_RELU, "leaky": ops_.ACT_LEAKY}[case.act]
        self.d = ops_.conv_desc(ops_.NHWC(self.xin, c=case.cin, coff=off), self.pk, ops_.NHWC(self.out, c=case.cout, coff=self.off),
                                stride=(stride, stride), dilation=(case.dil, case.dil), pad=(1, 1) if deconv else case.pad[:2], act=act,
                                slope=self.table.SLOPE, res=self.res)
        self.check_desc(_lib, ops_, self.d)

    def configure(self, hint, stage_k, split_k=-1, tail=(0, 0)):
        """Set the knobs and hand the descriptor exactly the workspace it then asks for (NaN-filled: a word read before it is written
        shows), inside a buffer with NaN words behind it.  -> the bytes asked for."""
        d = self.d
        d.tile_hint, d.stage_k, d.split_k, (d.tail_m_tiles, d.tail_split_k) = hint, stage_k, split_k, tail
        need = self.ops.workspace_bytes(d)
        assert need % 4 == 0
        self.ws = torch.full((need // 4 + GUARD_WORDS,), float("nan"), device="cuda") if need else None
        d.workspace, d.workspace_bytes = (self.ws.data_ptr(), need) if need else (None, 0)
        return need

    def window(self):
        """The output window as NCHW on the host, after asserting that nothing around it, and nothing of the input, was written."""
        torch.cuda.synchronize()
        check_unchanged(self.case.id, "input buffer", self.xin.cpu(), self.before)
        return extract_window(self.case.id, self.out.cpu(), self.off, self.case.cout).permute(0, 3, 1, 2).contiguous()

    def launch(self, name=None):
        """Launch as configured -> window().  With a name: the launch also wrote every word of the workspace it asked for and none
        behind (configure handed it exactly those)."""
        self.out.fill_(SENTINEL)
        self.ops.run_desc(self.d)
        got = self.window()
        if name is not None and self.ws is not None:
            check_workspace(f"{self.case.id} {name}", self.ws.cpu(), self.d.workspace_bytes // 4)
        return got

    def run_hint(self, hint, stage_k):
        """One launch of a kernel that asks for no workspace."""
        assert self.configure(hint, stage_k) == 0
        return self.launch()

    def refused(self, lib, stream):
        """Launch as configured; -> the error message, after asserting an error code, an untouched output and an untouched input."""
        self.out.fill_(SENTINEL)
        rc = lib.premvos_conv2d_f32(ctypes.byref(self.d), stream)
        torch.cuda.synchronize()
        assert rc != 0, self.case.id
        check_untouched(self.case.id, self.out.cpu())
        check_unchanged(self.case.id, "input buffer", self.xin.cpu(), self.before)
        return lib.premvos_last_error().decode()
