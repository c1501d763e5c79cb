"""Every kernel instantiation behind pmctf_ew_f32, pmctf_nearest_up2_nhwc_f32 and pmctf_pixel_shuffle2_nhwc_f32, reached by
name and bit for bit: each row of ew_census.EW runs its ops through the C entry on views into sentinel-filled buffers,
asserts WHICH kernel ran (ops.ew_last_launch() against the row's expected expression) and compares the whole output buffer
— the view, the sentinels around it and the elements between the written ones — with the numpy restatement that
test_ew_census_cpu.py pins to the torch operations.  uint32 patterns; NaN payloads of computed results exempt."""
import ctypes

import numpy as np
import pytest
import torch

import edge_values as ev
import ew_census as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rid", [r[0] for r in ec.EW])
def test_ew_row(cuda, rid):
    r = ec.row(rid)
    for data in ("specials", "normal"):
        for op in ec.ops_of(r):
            launched, got, want = ec.run_row(r, op, data, seed=op)
            what = f"{rid}: op {ec.NAMES[op]} on {data}"
            assert ec.parse_launch(launched)[0] == ec.expected_kernel(r, op), f"{what}: launched {launched!r}"
            count, first = ec.compare(got, want)
            assert count == 0, (f"{what} ({launched}): {count} elements of the output buffer differ; first at {first - ec.PAD} "
                                f"from the view's origin: got {int(got.view(np.uint32)[first]):#010x}, "
                                f"want {int(want.view(np.uint32)[first]):#010x}")


@pytest.mark.parametrize("rid", [c[0] for c in ec.COPIES])
def test_copy_row(cuda, rid):
    """nearest_up2 / pixel_shuffle2 choose the 16-byte form by C % 4 alone; every special pattern arrives unchanged"""
    from pMCTF.hip import lib, ops
    _, entry, (n, h, w, c), expected = next(x for x in ec.COPIES if x[0] == rid)
    cin = c if entry == "nearest_up2" else 4 * c
    x = ev.specials_plane((n, h, w, cin), seed=12)
    want = (x.repeat(2, axis=1).repeat(2, axis=2) if entry == "nearest_up2" else
            x.reshape(n, h, w, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, 2 * h, 2 * w, c))
    words = want.size
    buf = torch.full((words + 2 * ec.PAD,), ec.SENT, dtype=torch.int32, device="cuda")
    dx, out = torch.from_numpy(x).cuda(), ctypes.c_void_p(buf.data_ptr() + 4 * ec.PAD)
    if entry == "nearest_up2":
        rc = lib.hip().pmctf_nearest_up2_nhwc_f32(ctypes.c_void_p(dx.data_ptr()), out, n, h, w, c, None)
    else:
        rc = lib.hip().pmctf_pixel_shuffle2_nhwc_f32(ctypes.c_void_p(dx.data_ptr()), out, n, h, w, c, 0, 0.0, None)
    assert rc == 0
    assert ec.parse_launch(ops.ew_last_launch())[0] == expected
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:ec.PAD] == ec.SENT).all() and (got[ec.PAD + words:] == ec.SENT).all(), "wrote outside its output"
    assert (got[ec.PAD:ec.PAD + words] == np.ascontiguousarray(want).view(np.uint32).reshape(-1)).all()


def test_the_record_is_cleared_by_a_refused_call(cuda):
    from pMCTF.hip import lib, ops
    r = ec.row("flat_vec")
    launched, _, _ = ec.run_row(r, ec.EW_COPY, "normal")
    assert launched == ops.ew_last_launch() and launched.startswith(ec.FLAT_V + " grid ")
    x = torch.zeros(16, device="cuda")
    p = ctypes.c_void_p(x.data_ptr())
    assert lib.hip().pmctf_nearest_up2_nhwc_f32(p, p, 0, 1, 1, 1, None) == -1
    assert ops.ew_last_launch() == ""
