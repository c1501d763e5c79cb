"""Host threads: what the threaded tests share.  The rest of the suite drives every engine and the C ABI from
ONE host thread; the product also runs with several (bench.py --inflight, one model per thread behind CaptureGate, the
finishing threads of a decode).  Here: the barrier-started thread runner with its time limit and host intervals, the rows
the four threads of the C-ABI test walk (taken from the three censuses), and the inventory of what host threads share
(caches, per-thread and process-wide state of csrc/, streams and events of the engine), which
tests/test_host_threads_cpu.py holds against the source.

Importing this module needs neither the product nor a GPU.

    tests/host_threads_child.py      the fresh child processes: the C ABI from four threads, the engine cases
    tests/test_gpu_host_threads.py   starts them one at a time, and holds the caches to one object per key
    tests/test_host_threads_cpu.py   the inventory against the source
"""
import threading
import time

JOIN_S = 120.0                           # a thread that has not ended by then fails the run (a gate that never opens)


class Crew:
    """n host threads that stay: run(fns) hands fns[i] to thread i, releases all of them together through one barrier and
    waits for every result under a time limit.  The threads keep their identity from run to run (launch plans and the
    engine's count of host threads are keyed by it).  After a run that timed out the crew is `stuck`: the caller must
    not go on using the GPU."""

    def __init__(self, n):
        import queue
        self.n, self.stuck = n, False
        self.inbox = [queue.Queue() for _ in range(n)]
        self.outbox = queue.Queue()
        self.threads = [threading.Thread(target=self._body, args=(i,), name=f"host-thread-{i}", daemon=True)
                        for i in range(n)]
        for t in self.threads:
            t.start()

    def _body(self, i):
        while True:
            job = self.inbox[i].get()
            if job is None:
                return
            fn, barrier, limit = job
            try:
                barrier.wait(timeout=limit)
                self.outbox.put((i, fn(), None))
            except BaseException as e:  # noqa: BLE001 - reported by run(), on the caller's thread
                barrier.abort()
                self.outbox.put((i, None, e))

    def run(self, fns, limit=JOIN_S):
        """-> [result of fns[i]]; AssertionError naming the thread that raised, or the threads that did not end in time"""
        import queue
        assert len(fns) == self.n and not self.stuck
        barrier = threading.Barrier(self.n)
        for box, fn in zip(self.inbox, fns):
            box.put((fn, barrier, limit))
        end, got = time.monotonic() + limit, {}
        while len(got) < self.n:
            try:
                i, res, err = self.outbox.get(timeout=max(0.0, end - time.monotonic()))
            except queue.Empty:
                self.stuck = True
                raise AssertionError(f"host threads {sorted(set(range(self.n)) - set(got))} did not end within {limit} s")
            got[i] = (res, err)
        for i in range(self.n):
            if got[i][1] is not None:
                e = got[i][1]
                raise AssertionError(f"host thread {i}: {type(e).__name__}: {e}") from e
        return [got[i][0] for i in range(self.n)]

    def close(self, limit=10.0):
        for box in self.inbox:
            box.put(None)
        for t in self.threads:
            t.join(limit)
        self.stuck = self.stuck or any(t.is_alive() for t in self.threads)


def run_threads(fns, limit=JOIN_S):
    """fns[i]() on a fresh thread each, started together; joined under the time limit"""
    crew = Crew(len(fns))
    try:
        return crew.run(fns, limit)
    finally:
        if not crew.stuck:
            crew.close()


def pairwise_overlap(intervals):
    """intervals: one (t0, t1) per thread.  True when every two of them intersect: all threads were inside at once"""
    return all(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(intervals) for b in intervals[i + 1:])


# ----------------------------------------------------------------------------------------------- part 1: the C ABI rows
# Launch options of ONE call (ops.ConvLaunchOpts: split, msplit_px; < 0 = the process-wide knob).  NO_MSPLIT switches the
# cout-split small-plane path off for the call that carries it, which a census row can only do through the knob.
NO_MSPLIT = (-1, 0)

# What each of the four threads walks, round after round: (census, row id[, launch options]).  The process-wide knobs
# stay at their defaults throughout (a census row that needs another knob cannot run next to other threads), so a
# conv_census row is eligible if its knobs are empty, or are what launch options can say, and the defaults take the same
# path otherwise:
#   msplit_pipe33_mtp7_*   knobs {MSPLIT_PX: 2^40}: at the default 70 000 a plane of 962 pixels is cout-split all the same
#   pipe33_*_mt7           knobs {NT: 1, MSPLIT_PX: 0}: MSPLIT_PX travels with the launch; NT = 1 is what dispatch_tile
#                          takes for seven cout tiles below BIGPX anyway (its last `MTP >= 7` branch: launch<MTP, 1, 1>)
# Side by side (same round, same instant in the best case) run therefore
#   MFMA entry     thread 0 rule chain | thread 1 rule blocks | thread 2 reduce-32 | thread 3 both     (t_sum, g_last_launch)
#                  threads 1 and 3 with launch options, threads 0, 2 and 3 without; 0 and 3 on ONE geometry and rule
#   small-cin      thread 0 gemm | thread 1 gemv 3x3 | thread 2 blocks (strip) | thread 3 the dual entry        (g_valu_last)
#   elementwise    thread 0 flat | thread 1 c4 channels | thread 2 generic | thread 3 c4 rows                      (g_ew_last)
ROWS = [
    [("conv", "msplit_pipe33_mtp7_chain"), ("valu", "generic_gemm_cin3"), ("ew", "flat_vec")],
    [("conv", "pipe33_blocks_mt7", NO_MSPLIT), ("valu", "generic_gemv_cout16"), ("ew", "c4_channels")],
    [("conv", "gemm1x1_reduce32_nt2_cout64"), ("valu", "strip_cin1_cout32"), ("ew", "generic_cfast")],
    [("conv", "pipe33_chain_mt7", NO_MSPLIT), ("conv", "msplit_pipe33_mtp7_blocks"), ("valu", "dual_rule1_act3"),
     ("ew", "c4_rows")],
]
CONV_KNOBS_BY_OPTS = {"msplit_pipe33_mtp7_chain": {"MSPLIT_PX": 1 << 40}, "msplit_pipe33_mtp7_blocks": {"MSPLIT_PX": 1 << 40},
                      "pipe33_blocks_mt7": {"NT": 1, "MSPLIT_PX": 0}, "pipe33_chain_mt7": {"NT": 1, "MSPLIT_PX": 0},
                      "gemm1x1_reduce32_nt2_cout64": {}}
EW_OPS = (9, 16)                         # EW_ADD_MULS_MULS (binary) and EW_ROUND_CLAMP (unary) of every ew row
ROUNDS = 40                              # per thread: 4 threads x (4 or 5 calls) x 40 rounds = 680 calls, about a second
REFUSED_THREAD = 0                       # the thread that interleaves calls refused before any launch


# ------------------------------------------------------------------------------------- the inventory: engine caches
# every dict HipEngine.__init__ creates: name -> ("locked", the method that fills it under _cache_lock)
#                                             | ("per-thread" | "host-only", why no lock is needed)
ENGINE_CACHES = {
    "_convs": ("locked", "conv"),
    "_dw": ("locked", "dwconv"),
    "_lin": ("locked", "lin_tables"),
    "_dev_tab": ("locked", "_dev_tables"),
    "_llw": ("locked", "_ll_weights"),
    "_bitparm": ("locked", "bitparm_consts"),
    "tables": ("host-only", "host arrays of the entropy tables, filled in __init__ and only read afterwards"),
    "pair_plans": ("per-thread", "keyed by (thread id, shapes, ...): a thread meets its own plans only, and recording "
                                 "stops for good when a second thread enters (_gated)"),
    "_plan_ctx": ("per-thread", "keyed by thread id (plan_context): pools and streams of the calling thread's plans"),
    "stats": ("host-only", "host counters of the profile switch (profile_host); no device object"),
}

# --------------------------------------------------------- the inventory: per-thread and process-wide state of csrc/
# (file, name) -> kind.  Kinds: "thread_local" (one per calling host thread: the threads of part 1 differ in exactly
# these), "once_flag" (a first-use attribute setting, reached under contention by part 1's first round and by the K
# threads of part 3), "process-wide" (one value for all threads: read-only after first use, or a tuning knob that
# part 1 reads before and after), "function-static" (a switch read once per process from the environment).
C_STATE = {
    ("basic_ops.hip", "g_valu_last"): "thread_local",
    ("ew_ops.hip", "g_ew_last"): "thread_local",
    ("conv_mfma.hip", "t_sum"): "thread_local",
    ("conv_mfma.hip", "g_last_launch"): "thread_local",
    ("conv_mfma.hip", "g_last_len"): "thread_local",
    ("conv_mfma.hip", "g_knobs"): "process-wide",
    ("conv_mfma.hip", "g_knobs_once"): "once_flag",
}
for _n in ("once_t", "once_7b", "once_k4", "once_k3", "once_kb", "once_sb", "once_k", "once_w", "once_7", "once_p6",
           "once_p9", "once_s"):
    C_STATE[("conv_mfma.hip", _n)] = "once_flag"
C_STATE[("conv_split.hip", "once")] = "once_flag"              # two of this name, one per entry
for _n in ("once_r", "once", "once_b"):
    C_STATE[("decode_ops.hip", _n)] = "once_flag"
# function-static objects: C++ initialises each once, thread-safely, at the first call that reaches it.  The environment
# switches are read there (once per process: the censuses run their other setting in a child process); the others are
# constant tables, and pu_fused's `attr` is a first-use attribute setting in the same dress as a once_flag.
for _f, _n in (("basic_ops.hip", "use_lds"), ("basic_ops.hip", "column"), ("conv_split.hip", "forced"),
               ("decode_ops.hip", "v1"), ("decode_ops.hip", "v2"), ("decode_ops.hip", "one_thread"),
               ("conv_mfma.hip", "allowed"), ("decode_ops.hip", "TA"), ("decode_ops.hip", "TBT"), ("quality_ops.hip", "win"),
               ("pu_fused.hip", "attr")):
    C_STATE[(_f, _n)] = "function-static"
C_STATE[("pu_fused.hip", "pu_extra_lds")] = "process-wide"     # behind PMCTF_PU_PROFILE: not in the library the product loads

# ------------------------------------------------------------ the inventory: streams and events more than one thread reaches
# every attribute of HipEngine whose name says stream or event, or that holds one -> (what it is, the cases of part 3
# that reach it from several threads at once; none for what is no stream)
ENGINE_STREAMS = {
    "side_streams": ("shared streams: luma / chroma coders of a pair, the finishing threads of a decode (_finish_files)",
                     ("decoder_in_loop", "decode_files")),
    "batch_streams": ("shared streams: one per geometry group of a batched LL decode", ("decode_files",)),
    "motion_stream": ("shared stream: the motion chain of a stage-batched encode", ("batched",)),
    "lt_event": ("shared event behind the last batched luma lifting, replaced by every caller", ("batched",)),
    "lt_stream": ("the stream lt_event was recorded on, replaced with it", ("batched",)),
    "keep_streams": ("a flag (keep bytes and symbol traces), not a stream", ()),
    "multi_stream": ("a flag (luma / chroma on the two side streams), not a stream", ()),
    "multi_stream_max_pairs": ("a number, not a stream", ()),
    "_plan_ctx": ("per-thread plan streams (plan_context, keyed by thread id)", ("after_plans", "two_models")),
}
CASES = ("first_touch", "after_plans", "batched", "decoder_in_loop", "decode_files", "estimate", "two_models")
