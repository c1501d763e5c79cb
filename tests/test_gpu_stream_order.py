"""Every entry point of the C ABI honours the stream it is given (stream_order.ROWS): behind a bounded delay on
a stream of the test's own, with the inputs uploaded after the delay, each call reproduces the bits of the same call made
on the default stream with everything synchronised; the control of each row (the same sequence with the wrapper on the
default stream) does not, which is what shows that the row could have failed."""
import pytest
import torch

import stream_order as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def caller(cuda):
    """the caller's stream of every row: the first fresh stream with a window against the default stream, both ways"""
    s, report = so.pick_stream(cuda)
    print(f"\ncaller stream: candidate {report[-1][0]} of {len(report)}; windows (name, forward, back): {report}")
    return s


def test_the_delay_is_what_it_says(cuda):
    """one spin of KERNEL_DELAY_MS, timed with events: calibrated within a factor of two, and bounded"""
    st = torch.cuda.Stream(device=cuda)
    so.calibrate(cuda)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    so.delay(st, so.KERNEL_DELAY_MS)
    e1.record(st)
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    print(f"\ndelay({so.KERNEL_DELAY_MS}) took {ms:.2f} ms")
    assert so.KERNEL_DELAY_MS / 2 <= ms <= 2 * so.KERNEL_DELAY_MS
    assert so.KERNEL_DELAY_MS >= 3 * so.KERNEL_ENQUEUE_MS and so.KERNEL_DELAY_MS <= so.MAX_DELAY_MS
    with pytest.raises(AssertionError):
        so.delay(st, so.MAX_DELAY_MS + 1)


def test_the_window_check_tells_one_queue_from_two(cuda, caller):
    default = torch.cuda.default_stream(cuda)
    assert not so.window(caller, caller), "a stream reads its own marker in order"
    assert so.window(caller, default) and so.window(default, caller)


@pytest.mark.parametrize("row", so.ROWS, ids=[r.name.replace(" ", "_") for r in so.ROWS])
def test_entry_runs_in_its_stream_s_order(cuda, caller, row):
    so.check_row(row, cuda, caller)
