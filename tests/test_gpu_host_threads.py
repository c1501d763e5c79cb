"""Host threads: every threaded mode of the product against its serial run.

  part 1  the C ABI from four host threads at once, in one fresh child process (tests/host_threads_child.py abi): census
          rows that differ in exactly the per-thread state of csrc/, every output against the oracle's bits and every
          launch record against the row's, refused calls interleaved on one thread, the process-wide knobs unchanged
  part 2  one object per cache key, ever: four threads ask a fresh engine for the same key while the constructor the cache
          calls sleeps 20 ms; exactly one construction, and all four get the identical object
  part 3  the engine's threaded modes (bench.py --inflight, the decoder's callers, estimate mode, one model per thread
          behind CaptureGate) in fresh child processes with eight hardware queues, one child at a time, each under its own
          time limit: K caller threads, each with a stream and an output folder of its own, equal the same GOPs coded one
          after the other by one thread; overlap of the threads' host intervals is asserted, not hoped for"""
import json
import os
import subprocess
import sys
import threading
import time

import pytest

import host_threads as ht

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_threads_child.py")
# a child: interpreter and torch start-up, GPU initialisation, one to three models, its runs (DESIGN 6h has the seconds)
CHILD_TIMEOUT = 300
# cases by the models they share; the order is the order the children run in
GROUPS = {
    "one_model": ("after_plans", "batched", "decoder_in_loop", "estimate"),
    "fresh_model": ("first_touch",),
    "decode": ("decode_files",),
    "two_models": ("two_models",),
}
_abnormal = []                           # a child that ended abnormally: no further child is started


def _child(args, tmp_path, env=None):
    if _abnormal:
        pytest.fail(f"not started: the child {_abnormal[0]} ended abnormally")
    result = str(tmp_path / "result.json")
    cmd = [sys.executable, CHILD] + [result if a == "RESULT" else a for a in args]
    t0 = time.time()
    try:
        p = subprocess.run(cmd, env=env or dict(os.environ), timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired as e:
        _abnormal.append(" ".join(args))
        pytest.fail(f"{args}: no exit within {CHILD_TIMEOUT} s\n{(e.stdout or '')[-3000:]}")
    if p.returncode not in (0, 1) or not os.path.exists(result):
        _abnormal.append(" ".join(args))
        pytest.fail(f"{args}: the child ended with status {p.returncode}\n{p.stdout[-4000:]}")
    out = json.load(open(result))
    print(f"\n{' '.join(args[:2])}: {time.time() - t0:.1f} s\n{json.dumps(out, indent=1)[:6000]}")
    assert out["ok"], f"{args}: {out.get('error')}\n{out.get('trace', '')}\n{p.stdout[-2000:]}"
    return out


def test_the_c_abi_from_four_host_threads(cuda, tmp_path):
    """part 1"""
    out = _child(["abi", "RESULT"], tmp_path)
    assert out["knobs_unchanged"] and len(out["threads"]) == 4
    for i, rep in enumerate(out["threads"]):
        want = [r[1] for r in ht.ROWS[i] if r[0] != "ew"]
        assert [r for r in rep["rows"] if ":" not in r] == want and rep["rounds"] == ht.ROUNDS
        assert rep["calls"] == ht.ROUNDS * len(rep["rows"]) and rep["mismatches"] == 0
        assert rep["refused"] == (rep["calls"] if i == ht.REFUSED_THREAD else 0)


@pytest.mark.parametrize("group", list(GROUPS))
def test_threaded_modes_equal_their_serial_runs(cuda, tmp_path, group):
    """part 3"""
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    out = _child(["engine", group, "RESULT", str(scratch)], tmp_path, dict(os.environ, GPU_MAX_HW_QUEUES="8"))
    assert sorted(k for k in out if k not in ("ok", "total_seconds")) == sorted(GROUPS[group])
    for case in GROUPS[group]:
        runs = out[case]["runs"]
        assert runs and all(len(v) >= 3 and v[0]["delayed"] is None and all(o > 0 for r in v for o in r["overlap_ms"])
                            for v in runs.values()), runs


# ---------------------------------------------------------------------------------------------------------------- part 2
SLEEP_S = 0.020


@pytest.fixture(scope="module")
def fresh(cuda):
    """a model whose engine has built nothing yet"""
    from helpers import product_model
    net, _ = product_model(1)
    return net


class Counted:
    """wraps a constructor or an upload: counts the calls per key and sleeps on the host before it returns"""

    def __init__(self, fn, key):
        self.fn, self.key, self.calls, self.lock = fn, key, {}, threading.Lock()

    def __call__(self, *a, **k):
        out = self.fn(*a, **k)
        key = self.key(*a, **k)
        with self.lock:
            self.calls[key] = self.calls.get(key, 0) + 1
        time.sleep(SLEEP_S)
        return out


def _cache_cases(net):
    """name -> (what to patch: (object, attribute, key function), the call every thread makes, the cache, its key)"""
    import torch
    from pMCTF.hip import lib, ops
    eng = net.engine()
    conv_p = next(k[:-7] for k, v in eng.sd.items() if k.endswith(".weight") and v.dim() == 4 and v.shape[1] >= 16
                  and v.shape[2] == 3)
    dw_p = next(k[:-7] for k, v in eng.sd.items() if k.endswith(".depth_conv.weight") and v.dim() == 4 and v.shape[1] == 1)
    shape = lambda w, *a, **k: tuple(w.shape)
    return {
        "conv": ((ops, "Conv2d", shape), lambda: eng.conv(conv_p, 1, 1), eng._convs, (conv_p, 1, 1)),
        "dwconv": ((ops, "DepthwiseConv2d", shape), lambda: eng.dwconv(dw_p), eng._dw, dw_p),
        "lin_tables": ((torch, "linspace", lambda lo, hi, n, **k: n), lambda: eng.lin_tables(36, 52), eng._lin, (36, 52)),
        "_dev_tables": ((torch, "from_numpy", lambda a: (a.shape, a.ctypes.data)), lambda: eng._dev_tables("gauss"), eng._dev_tab, "gauss"),
        "_ll_weights": ((lib.hip(), "pmctf_ll_ar_pack_weights", lambda *a: "pack"), lambda: eng._ll_weights("hp_coder"),
                        eng._llw, "hp_coder"),
        "bitparm_consts": ((torch, "stack", lambda rows, **k: len(rows)), lambda: eng.bitparm_consts(0), eng._bitparm, 0),
    }


CACHES = ("conv", "dwconv", "lin_tables", "_dev_tables", "_ll_weights", "bitparm_consts")


@pytest.mark.parametrize("name", CACHES)
def test_one_object_per_cache_key_ever(cuda, fresh, monkeypatch, name):
    """four threads miss together; the constructor sleeps 20 ms: one construction, one object (no timing luck: without
    the lock every thread is inside the constructor before the first one returns)"""
    import torch
    (obj, attr, key), ask, cache, ckey = _cache_cases(fresh)[name]
    assert ckey not in cache, "the engine is fresh for this key"
    counted = Counted(getattr(obj, attr), key)
    monkeypatch.setattr(obj, attr, counted)

    def thread():
        torch.cuda.set_device(cuda)
        return ask()
    got = ht.run_threads([thread] * 4, limit=60.0)
    monkeypatch.undo()
    torch.cuda.synchronize()
    print(f"\n{name}: constructions per key {counted.calls}")
    assert counted.calls and set(counted.calls.values()) == {1}, f"{name}: constructions per key {counted.calls}"
    assert all(g is got[0] for g in got), f"{name}: the threads hold different objects"
    assert cache[ckey] is got[0]
