"""pmgt_op_cls_gather / pmgt_op_cls_scatter: the glue between the encoder's last_hidden_state [n, S, d] (engine dtype) and the fp32 rows
[n, d] of the head that is fine-tuned with it.  Copies and one rounding: everything is asserted BIT FOR BIT against torch -- the gather
against last[:, 0].float(), the scatter (into a NaN-filled buffer: it must be written whole) against a zero tensor with
[:, 0] = d_item.to(dtype), the sign bit of the zeros included.  Shapes: one element group, several blocks, d = 256, and d = 20, which is
no multiple of 8 and takes the element-wise kernels; a misaligned view of the same data takes them too."""
import ctypes as C

import pytest
import torch

from pmgt_amd import _lib

pytestmark = pytest.mark.gpu

DT = {"fp32": (_lib.DTYPE_F32, torch.float32, torch.int32), "bf16": (_lib.DTYPE_BF16, torch.bfloat16, torch.int16)}
SHAPES = [(1, 1, 8), (33, 16, 64), (257, 32, 256), (5, 3, 20)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t, as_int):
    return t.contiguous().view(as_int)


def inputs(n, S, d, tdt):
    g = torch.Generator().manual_seed(n * 1000 + S * 10 + d)
    last = (torch.randn(n, S, d, generator=g) * 3).to(tdt)
    d_item = torch.randn(n, d, generator=g) * 1e-2
    d_item[0, 0], d_item[-1, -1] = -0.0, 1e-41               # a negative zero and a subnormal (bf16: rounds to a subnormal or to zero, as torch's)
    return last.cuda(), d_item.cuda()


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("n,S,d", SHAPES)
def test_gather_is_the_cls_row_as_fp32(n, S, d, dt):
    code, tdt, _ = DT[dt]
    last, _ = inputs(n, S, d, tdt)
    x = torch.full((n + 1, d), float("nan"), device="cuda")
    _lib.check(_lib.hip().pmgt_op_cls_gather(code, last.data_ptr(), n, S, d, x.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(x[:n], torch.int32), bits(last[:, 0].float(), torch.int32))
    assert torch.isnan(x[n]).all()                           # nothing past row n


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("n,S,d", SHAPES)
def test_scatter_writes_the_whole_gradient(n, S, d, dt):
    code, tdt, as_int = DT[dt]
    _, d_item = inputs(n, S, d, tdt)
    out = torch.full((n + 1, S, d), float("nan"), device="cuda", dtype=tdt)
    _lib.check(_lib.hip().pmgt_op_cls_scatter(code, d_item.data_ptr(), n, S, d, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    want = torch.zeros(n, S, d, device="cuda", dtype=tdt)
    want[:, 0] = d_item.to(tdt)
    assert torch.equal(bits(out[:n], as_int), bits(want, as_int))
    assert torch.isnan(out[n].float()).all()


@pytest.mark.parametrize("dt", list(DT))
def test_misaligned_buffers_take_the_element_kernels(dt):
    """d a multiple of 8 but pointers 4 (fp32) or 2 (bf16) bytes off a 16-byte boundary: the same results through the other kernels"""
    code, tdt, as_int = DT[dt]
    n, S, d = 9, 4, 16
    last, d_item = inputs(n, S, d, tdt)
    off_last = torch.empty(last.numel() + 1, device="cuda", dtype=tdt)[1:].view(n, S, d)
    off_last.copy_(last)
    x = torch.full((n * d + 1,), float("nan"), device="cuda")[1:].view(n, d)
    _lib.check(_lib.hip().pmgt_op_cls_gather(code, off_last.data_ptr(), n, S, d, x.data_ptr(), stream()))
    out = torch.full((n * S * d + 1,), float("nan"), device="cuda", dtype=tdt)[1:].view(n, S, d)
    off_item = torch.empty(n * d + 1, device="cuda")[1:].view(n, d)
    off_item.copy_(d_item)
    _lib.check(_lib.hip().pmgt_op_cls_scatter(code, off_item.data_ptr(), n, S, d, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(bits(x, torch.int32), bits(last[:, 0].float(), torch.int32))
    want = torch.zeros(n, S, d, device="cuda", dtype=tdt)
    want[:, 0] = d_item.to(tdt)
    assert torch.equal(bits(out, as_int), bits(want, as_int))


def test_refusals():
    lib = _lib.hip()
    a, b = torch.zeros(64, device="cuda"), torch.full((64,), float("nan"), device="cuda")
    bad = [lib.pmgt_op_cls_gather(2, a.data_ptr(), 1, 1, 8, b.data_ptr(), stream()), lib.pmgt_op_cls_gather(0, None, 1, 1, 8, b.data_ptr(), stream()),
           lib.pmgt_op_cls_gather(0, a.data_ptr(), 1, 1, 8, None, stream()), lib.pmgt_op_cls_gather(0, a.data_ptr(), 0, 1, 8, b.data_ptr(), stream()),
           lib.pmgt_op_cls_scatter(0, a.data_ptr(), 1, 0, 8, b.data_ptr(), stream()), lib.pmgt_op_cls_scatter(0, a.data_ptr(), 1, 1, 0, b.data_ptr(), stream()),
           lib.pmgt_op_cls_scatter(7, a.data_ptr(), 1, 1, 8, b.data_ptr(), stream()), lib.pmgt_op_cls_scatter(1, None, 1, 1, 8, b.data_ptr(), stream())]
    assert bad == [-2] * len(bad)
    torch.cuda.synchronize()
    assert torch.isnan(b).all()
