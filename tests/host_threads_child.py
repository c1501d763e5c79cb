"""The fresh child processes of tests/test_gpu_host_threads.py; not collected by pytest.

    python host_threads_child.py abi RESULT.json
        part 1: the C ABI from four host threads, each with a stream of its own and a disjoint list of census rows
        (host_threads.ROWS).  The first launch of every kernel, with its attribute setting under a once_flag, happens
        here under contention.  After every call: the output against the oracle's bits, the launch record of the calling
        thread against the row's.  One thread interleaves calls that are refused before any launch.

    python host_threads_child.py engine GROUP RESULT.json SCRATCH
        part 3: the cases of a group (GROUPS below: cases that can share models), each coded once by one thread on the
        default stream (the baseline) and then by K caller threads at once, each with a stream and an output folder of its
        own: once plain, then once per thread with a bounded delay in front of that thread's stream.  Every file byte,
        bit count and returned tensor must be the baseline's, and the threads' host intervals must pairwise intersect.

A child writes RESULT.json ({"ok": true, ...figures} or {"ok": false, "error": ...}) and exits with status 0 / 1; after a
thread that did not end within its time limit it starts nothing more on the GPU and leaves through os._exit(3)."""
import ctypes as C
import json
import os
import sys
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "learned-pmctf_amd"), os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import host_threads as ht  # noqa: E402

W, H, GOP, Q = 132, 100, 4, 3                            # the geometry of the stream-order engine cases: padded to 256x128
K = 3                                                    # caller threads
SEEDS = (41, 43, 47, 53)                                 # GOPs of different content: one per thread (two_models: two per model)
GROUPS = {
    "one_model": ("after_plans", "batched", "decoder_in_loop", "estimate"),
    "fresh_model": ("first_touch",),
    "decode": ("decode_files",),
    "two_models": ("two_models",),
}


class Stuck(Exception):
    """a host thread did not end within its time limit"""


# ===================================================================================================== part 1: the C ABI
def _prepare_abi():
    """host data and the oracle's expectation of every row, computed once, on the CPU"""
    import conv_census as cc
    import ew_census as ec
    import test_gpu_conv_census as tcc
    import valu_conv_census as vc
    prepared = []
    for rows in ht.ROWS:
        mine = []
        for item in rows:
            kind, rid = item[0], item[1]
            if kind == "conv":
                r = cc.row(rid)
                x, w, b, res = cc.case_data(r)
                mine.append({"kind": kind, "id": rid, "row": r, "data": (x, w, b, res), "want": tcc.reference(r, x, w, b, res),
                             "opts": item[2] if len(item) > 2 else None})
            elif kind == "valu":
                r = vc.row(rid)
                want, ok, text = vc.reference(r)
                assert ok, text
                mine.append({"kind": kind, "id": rid, "row": r, "want": want})
            else:
                r = ec.row(rid)
                for op in ht.EW_OPS:
                    bufs = ec.operands(r, "normal", seed=op)
                    mine.append({"kind": kind, "id": f"{rid}:{ec.NAMES[op]}", "row": r, "op": op, "bufs": bufs,
                                 "want": ec.reference(r, op, bufs)})
        prepared.append(mine)
    return prepared


def _bits_equal(got, want, what):
    import numpy as np
    got, want = (np.ascontiguousarray(a, dtype=np.float32) for a in (got, want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    neq = got.view(np.uint32) != want.view(np.uint32)
    assert not neq.any(), f"{what}: {int(neq.sum())}/{got.size} bit patterns differ from the oracle's; first at " \
                          f"{tuple(int(v) for v in np.argwhere(neq)[0])}"


def _walk(i, items, dev):
    """thread i: its rows, ROUNDS times, on a stream of its own -> report"""
    import numpy as np
    import torch
    import conv_census as cc
    import ew_census as ec
    import valu_conv_census as vc
    from pMCTF.hip import lib, ops
    L = lib.hip()
    torch.cuda.set_device(dev)
    S = torch.cuda.Stream(device=dev)
    st = C.c_void_p(S.cuda_stream)
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(dev)
    convs, calls, refused, t0 = {}, 0, 0, time.perf_counter()
    valid = torch.zeros(16, dtype=torch.float32, device=dev)
    p = C.c_void_p(valid.data_ptr())
    # refused on the host before any launch (tests/test_product_cpu.py: null pointers; N <= 0 with a valid pointer)
    refusals = [
        lambda: L.pmctf_conv2d_nhwc_f32(None, None, None, None, None, None, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0, 0.0, st),
        lambda: L.pmctf_flow_warp_f32(None, None, None, None, None, 1, 1, 8, 8, 1, 1.0, st),
        lambda: L.pmctf_math_probe_f32(0, None, 0, 16, None, 0.0, st),
        lambda: L.pmctf_math_probe_f32(0, None, 0, 0, p, 0.0, st),
        lambda: L.pmctf_math_probe_f32(0, None, 0, -1, p, 0.0, st),
        lambda: L.pmctf_nearest_up2_nhwc_f32(p, p, 0, 1, 1, 1, st),
        lambda: L.pmctf_dwconv2d_nhwc_f32(p, p, None, p, 0, 2, 2, 4, 3, st),
    ]
    with torch.cuda.stream(S), torch.no_grad():
        for rnd in range(ht.ROUNDS):
            for it in items:
                what = f"thread {i} round {rnd} {it['kind']} {it['id']}"
                if it["kind"] == "conv":
                    rid, (N, Cin, Hh, Ww, Cout, Kk, Sd, pad), rule, act, slope, nres, knobs, expected = it["row"]
                    x, w, b, res = it["data"]
                    if rid not in convs:
                        convs[rid] = ops.Conv2d(torch.from_numpy(w), None if b is None else torch.from_numpy(b), Sd, (pad, pad),
                                                rule=rule)
                        assert not convs[rid].small and not convs[rid].few and not convs[rid].split
                    xd, rd = nhwc(x), [nhwc(q) for q in res]
                    with ops.launch_opts(ops.ConvLaunchOpts(*it["opts"]) if it["opts"] else None):
                        y = convs[rid](xd, act=act, slope=slope, res1=rd[0] if nres > 0 else None,
                                       res2=rd[1] if nres > 1 else None)
                    buf = C.create_string_buffer(512)
                    assert L.pmctf_conv2d_last_launch(buf, 512) == 0
                    launched = buf.value.decode()
                    S.synchronize()
                    assert cc.parse_launch(launched) == expected, f"{what}: record {launched!r}, expected {expected}"
                    _bits_equal(np.ascontiguousarray(y.cpu().numpy().transpose(0, 3, 1, 2)), it["want"], f"{what} ({launched})")
                elif it["kind"] == "valu":
                    outs, launched, intact = vc.run_row(it["row"])
                    assert launched == ops.valu_conv_last_launch(), what
                    assert vc.parse_launch(launched)[0] == it["row"][9], f"{what}: record {launched!r}, expected {it['row'][9]}"
                    assert intact, f"{what}: a store outside the output"
                    assert len(outs) == len(it["want"])
                    for got, want in zip(outs, it["want"]):
                        _bits_equal(got, want, f"{what} ({launched})")
                else:
                    r, op = it["row"], it["op"]
                    d = r[1]
                    devb = {k: torch.from_numpy(v.copy()).to(dev) for k, v in it["bufs"].items()}
                    ptr = lambda view: C.c_void_p(devb[view[0]].data_ptr() + 4 * (ec.PAD + view[1]))
                    i64x4 = C.c_int64 * 4
                    binary = op in ec.BINARY
                    alpha, beta = ec.params(op)
                    rc = L.pmctf_ew_f32(op, ptr(r[3]), i64x4(*r[3][2]), ptr(r[4]), i64x4(*r[4][2]), ptr(r[5]) if binary else None,
                                        i64x4(*r[5][2]) if binary else None, *d, alpha, beta, r[2], st)
                    assert rc == 0, (what, rc)
                    launched = ops.ew_last_launch()
                    S.synchronize()
                    assert ec.parse_launch(launched)[0] == ec.expected_kernel(r, op), f"{what}: record {launched!r}"
                    count, first = ec.compare(devb["out"].cpu().numpy(), it["want"])
                    assert count == 0, f"{what} ({launched}): {count} elements of the output buffer differ, first at {first}"
                calls += 1
                if i == ht.REFUSED_THREAD:
                    rc = refusals[refused % len(refusals)]()
                    assert rc == -1, f"{what}: refused call {refused % len(refusals)} returned {rc}, not PMCTF_EINVAL"
                    refused += 1
        S.synchronize()
    return {"thread": i, "rows": [it["id"] for it in items], "rounds": ht.ROUNDS, "calls": calls, "refused": refused,
            "mismatches": 0, "seconds": round(time.perf_counter() - t0, 3)}


def abi():
    import torch
    import conv_census as cc
    from pMCTF.hip import lib
    prepared = _prepare_abi()
    L = lib.hip()
    dev = torch.device("cuda:0")
    torch.cuda.init()
    torch.zeros(1, device=dev)
    before = {k: L.pmctf_conv2d_get_option(k.encode()) for k in cc.KNOBS}
    assert all(v == cc.KNOBS[k] for k, v in before.items() if f"PMCTF_CONV_{k}" not in os.environ), "the rows expect the defaults"
    crew = ht.Crew(len(prepared))
    t0 = time.perf_counter()
    try:
        reports = crew.run([lambda i=i: _walk(i, prepared[i], dev) for i in range(len(prepared))])
    except AssertionError:
        if crew.stuck:
            raise Stuck(traceback.format_exc())
        raise
    finally:
        if not crew.stuck:
            crew.close()
    wall = time.perf_counter() - t0
    torch.cuda.synchronize(dev)
    after = {k: L.pmctf_conv2d_get_option(k.encode()) for k in cc.KNOBS}
    assert after == before, {k: (before[k], after[k]) for k in before if before[k] != after[k]}
    return {"threads": reports, "wall_seconds": round(wall, 3), "knobs_unchanged": True}


# ================================================================================================ part 3: the engine cases
def _cpu(t):
    """a copy on the calling thread's current stream, finished when it returns"""
    t = t.force() if hasattr(t, "force") else t
    return t.detach().to("cpu")


def _harvest(enc):
    out = {}
    for i, fc in enumerate(enc["frames_coded"]):
        for j, t in enumerate(fc):
            if t is not None:
                out[f"frame{i} tensor{j}"] = _cpu(t)
    for i, r in enumerate(enc.get("results", ())):
        for k in ("mv_feature", "ref_mv_y"):
            out[f"pair{i} dpb {k}"] = _cpu(r["dpb"][k])
    out["bits"] = repr((enc["bits"], enc["bits_mv"]))
    return out


def _as_bytes(out, folder=None):
    import torch
    res = {k: (v.contiguous().numpy().tobytes() if isinstance(v, torch.Tensor) else repr(v).encode()) for k, v in out.items()}
    if folder is not None:
        for name in sorted(os.listdir(folder)):
            res[f"file {name}"] = open(os.path.join(folder, name), "rb").read()
    return res


def _same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want)))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} files, bit counts and tensors differ from the serial run: {bad[:8]}"


class Rig:
    def __init__(self, scratch):
        import torch
        import stream_order as so
        from helpers import frames
        self.dev = torch.device("cuda:0")
        torch.cuda.set_device(self.dev)
        self.scratch, self.n, self.so, self.sd = scratch, 0, so, None
        self.pinned = [[[t.pin_memory() for t in f] for f in frames(W, H, GOP, seed=s)] for s in SEEDS]
        so.calibrate(self.dev)                               # the delays' spin rate: once, on the main thread
        self.figures = {}
        self.crew = ht.Crew(K)

    def model(self, plans):
        """helpers.product_model(1); the synthetic weights are drawn once per process"""
        from helpers import product_model
        if self.sd is None:
            net, self.sd = product_model(1)
        else:
            from pMCTF.models.video.pMCTF_L import pMCTF
            net = pMCTF(num_me_stages=1).eval()
            net.load_state_dict(self.sd, strict=True)
            net = net.to(self.dev)
            net.update(force=True)
            net.lazy_stages = False
        eng = net.engine()                                   # as bench.py --inflight: the engine exists before the threads
        eng.use_graphs = plans
        return net

    def folder(self, tag):
        self.n += 1
        path = os.path.join(self.scratch, f"{self.n:03d}_{tag}")
        os.makedirs(path)
        return path

    def pictures(self, g):
        return [[t.to(self.dev, non_blocking=True) for t in f] for f in self.pinned[g]]

    def run(self, crew, fns, limit=ht.JOIN_S):
        try:
            return crew.run(fns, limit)
        except AssertionError:
            if crew.stuck:
                raise Stuck(traceback.format_exc())
            raise


def _encode(net, mode, pics, folder):
    import pmctf_gop
    if mode == "batched":
        enc = pmctf_gop.encode_gop_batched(net, pics, H, W, Q, folder)
    else:
        enc = pmctf_gop.encode_gop(net, pics, H, W, Q, folder, skip_decoding=mode != "decoder")
    net.flush()
    return enc


def serial_encode(rig, net, mode, gops, keep=None):
    """the baseline: the GOPs one after the other, one thread, the default stream -> [{name: bytes}] per GOP"""
    import torch
    out = []
    with torch.no_grad():
        for g in gops:
            folder = rig.folder(f"serial_{mode}_gop{g}")
            enc = _encode(net, mode, rig.pictures(g), folder)
            out.append(_as_bytes(_harvest(enc), folder))
            if keep is not None:
                keep.append((folder, enc))
    torch.cuda.synchronize(rig.dev)
    return out


def threaded(rig, crew, jobs, delayed, ms, tag):
    """jobs[k](S, g) -> harvest of thread k's unit g, run under the thread's own stream S; every thread runs len(units)
    units, with a barrier in front of each, and notes its host interval per unit.  delayed: the thread whose stream gets
    a delay of `ms` in front of every unit (None: nobody).  -> ([[harvest per unit] per thread], intervals[k][g])"""
    import threading
    import torch
    n = len(jobs)
    units = len(jobs[0][1])
    gates = [threading.Barrier(n) for _ in range(units)]

    def body(k):
        fn, mine = jobs[k]
        torch.cuda.set_device(rig.dev)
        S = torch.cuda.Stream(device=rig.dev)
        got, spans = [], []
        with torch.no_grad(), torch.cuda.stream(S):
            for u, g in enumerate(mine):
                gates[u].wait(timeout=ht.JOIN_S)
                if delayed == k:
                    assert not torch.cuda.is_current_stream_capturing()
                    rig.so.delay(S, ms)
                t0 = time.perf_counter()
                got.append(fn(S, g))
                spans.append((t0, time.perf_counter()))
            S.synchronize()
        return got, spans
    res = rig.run(crew, [lambda k=k: body(k) for k in range(n)])
    spans = [r[1] for r in res]
    for u in range(units):
        iv = [spans[k][u] for k in range(n)]
        assert ht.pairwise_overlap(iv), f"{tag}: unit {u}: the threads' host intervals do not pairwise intersect " \
                                        f"({[(round(a, 3), round(b, 3)) for a, b in iv]}): unexercised"
    rig.figures.setdefault(tag.split(",")[0], []).append(
        {"delayed": delayed, "host_ms": [[round((b - a) * 1e3, 1) for a, b in spans[k]] for k in range(n)],
         "overlap_ms": [round((min(spans[k][u][1] for k in range(n)) - max(spans[k][u][0] for k in range(n))) * 1e3, 1)
                        for u in range(units)]})
    return [r[0] for r in res]


def encode_case(rig, net, mode, delay_key, want, tag, after=None):
    """K threads code GOP k each through `mode` on `net`: plain, then delayed per thread; all against `want`"""
    ms = rig.so.ENGINE_DELAY_MS[delay_key]
    assert 0 < ms <= rig.so.MAX_DELAY_MS
    for delayed in (None,) + tuple(range(K)):
        folders = [rig.folder(f"{tag}_t{k}") for k in range(K)]

        def job(k):
            return lambda S, g: _harvest(_encode(net, mode, rig.pictures(g), folders[k]))
        got = threaded(rig, rig.crew, [(job(k), [k]) for k in range(K)], delayed, ms, f"{tag}, delayed {delayed}")
        for k in range(K):
            _same(_as_bytes(got[k][0], folders[k]), want[k], f"{tag}, thread {k}, delayed thread {delayed}")
        if after is not None:
            after(delayed)


class Replays:
    """counts PairPlan.run while it is open"""

    def __enter__(self):
        from pMCTF.hip import pair_plan
        self.n, self.mod, self.orig = 0, pair_plan, pair_plan.PairPlan.run
        orig, me = self.orig, self

        def counted(plan, *a, **k):
            me.n += 1
            return orig(plan, *a, **k)
        pair_plan.PairPlan.run = counted
        return self

    def __exit__(self, *exc):
        self.mod.PairPlan.run = self.orig


def case_after_plans(rig, shared):
    """case 1a: the threads arrive on a model that has recorded and replayed its plans from one thread"""
    net = shared["net"] = rig.model(plans=True)
    eng = net.engine()
    with Replays() as rp:
        want = shared["pairs"] = serial_encode(rig, net, "pairs", range(K))      # GOP 0 records, GOPs 1 and 2 replay
    assert eng.use_graphs and len(eng.pair_plans) >= 2 and rp.n == 3 * (K - 1), (eng.use_graphs, len(eng.pair_plans), rp.n)
    assert len({w["file 1.bin"] for w in want}) == K, "the GOPs must differ"
    with Replays() as rp:
        encode_case(rig, net, "pairs", "plans_off", want, "after_plans")
    assert rp.n == 0, f"{rp.n} plan replays with several host threads in the engine"
    assert eng.use_graphs is False and len(eng.host_threads) == K + 1
    return {"replays_serial": 3 * (K - 1), "replays_threaded": 0, "plans_kept": len(eng.pair_plans)}


def case_first_touch(rig, shared):
    """case 1b: the threads arrive on a model that never ran (every cache is filled under contention)"""
    ref = rig.model(plans=False)
    want = serial_encode(rig, ref, "pairs", range(K))
    net = rig.model(plans=False)
    eng = net.engine()
    assert not eng._convs and not eng._dw and not eng._lin and not eng.host_threads
    state = {}

    def after(delayed):
        if delayed is None:
            state["convs"] = {k: id(v) for k, v in eng._convs.items()}
            assert len(state["convs"]) > 20
        else:
            assert {k: id(v) for k, v in eng._convs.items()} == state["convs"], "a cached layer was replaced"
    encode_case(rig, net, "pairs", "plans_off", want, "first_touch", after)
    return {"layers_cached": len(state["convs"])}


def case_batched(rig, shared):
    """case 2: encode_gop_batched: the shared motion stream and the lt_event / lt_tensor snapshot"""
    net = shared["net"]
    assert net.engine().motion_overlap
    want = serial_encode(rig, net, "batched", range(K))
    for k in range(K):
        files = lambda d: {n: v for n, v in d.items() if n.startswith("file ")}
        _same(files(want[k]), files(shared["pairs"][k]), f"stage-batched against pair by pair, GOP {k}")
    encode_case(rig, net, "batched", "batched", want, "batched")
    return {}


def case_decoder_in_loop(rig, shared):
    """case 3: encode_gop(skip_decoding=False): shared side streams and finishing threads for K pairs at once"""
    net = shared["net"]
    want = serial_encode(rig, net, "decoder", range(K))
    encode_case(rig, net, "decoder", "decoder", want, "decoder_in_loop")
    eng = net.engine()
    assert eng._batch_pool is not None and len(eng.side_streams) >= 2
    return {}


def _estimate(net, pics):
    dpb = {"mv_feature": None, "ref_mv_y": None}
    (y0, c0), (y1, c1) = pics[0], pics[1]
    ry = net.forward_one_stage(y0, y1, Q, True, dpb)
    rc = net.forward_one_stage(c0, c1, Q, True, dpb, mv_hat=ry["mv_hat"])
    out = {}
    import torch
    for tag, r in (("y", ry), ("c", rc)):
        for k, v in r.items():
            if k == "dpb":
                for kk, t in v.items():
                    out[f"{tag} dpb.{kk}"] = None if t is None else _cpu(t)
            elif v is None or isinstance(v, torch.Tensor) and v.numel() > 1 or hasattr(v, "force"):
                out[f"{tag} {k}"] = None if v is None else _cpu(v)
            else:
                out[f"{tag} {k}"] = float(v)
    return out


def case_estimate(rig, shared):
    """case 5: estimate mode from K threads.  Tensors bit for bit; the totals as test_estimate_mode_forward compares its
    totals (1e-6 relative: the float64 atomics arrive in any order)"""
    import torch
    net = shared["net"]
    with torch.no_grad():
        want = [_estimate(net, rig.pictures(g)) for g in range(K)]
    torch.cuda.synchronize(rig.dev)
    n_scalars = sum(isinstance(v, float) for v in want[0].values())
    assert n_scalars >= 10 and any(isinstance(v, torch.Tensor) for v in want[0].values()), sorted(want[0])
    ms = rig.so.ENGINE_DELAY_MS["plans_off"]
    for delayed in (None,) + tuple(range(K)):
        got = threaded(rig, rig.crew, [(lambda S, g: _estimate(net, rig.pictures(g)), [k]) for k in range(K)], delayed, ms,
                       f"estimate, delayed {delayed}")
        for k in range(K):
            g, w = got[k][0], want[k]
            assert sorted(g) == sorted(w)
            for name, wv in w.items():
                what = f"estimate, thread {k}, delayed thread {delayed}, {name}"
                if isinstance(wv, float):
                    assert abs(g[name] - wv) <= 1e-6 * max(1.0, abs(wv)), (what, g[name], wv)
                elif wv is None:
                    assert g[name] is None, what
                else:
                    assert g[name].shape == wv.shape and g[name].numpy().tobytes() == wv.numpy().tobytes(), what
    return {"scalars": n_scalars}


def case_decode_files(rig, shared):
    """case 4: decode_gop_files from K caller threads on K folders of one model, in both LL orders, the first run on a
    model that never ran; and decode_gop on the coded tensors"""
    import torch
    import pmctf_gop
    enc_net = rig.model(plans=False)
    kept = {"plane": [], "position": []}
    serial_encode(rig, enc_net, "pairs", range(K), kept["plane"])                # skip_decoding=True: plane order
    serial_encode(rig, enc_net, "decoder", range(K), kept["position"])           # decoder order
    net = rig.model(plans=False)
    assert not net.engine()._convs and not net.engine()._llw and not net.engine()._dev_tab

    def decode(folder, order, codec):
        dec = pmctf_gop.decode_gop_files(codec, folder, GOP, H, W, Q, ll_order=order)
        return {f"frame{i} plane{j}": _cpu(t) for i, f in enumerate(dec["frames"]) for j, t in enumerate(f[:2])}

    def synth(enc, codec):
        rec = pmctf_gop.decode_gop(codec, [list(fc) for fc in enc["frames_coded"]])
        return {f"frame{i} plane{j}": _cpu(t) for i, f in enumerate(rec) for j, t in enumerate(f[:2])}
    ms = rig.so.ENGINE_DELAY_MS["decode"]
    out = {}
    for order in ("plane", "position"):
        with torch.no_grad():
            want = [_as_bytes(decode(folder, order, enc_net)) for folder, _ in kept[order]]
        torch.cuda.synchronize(rig.dev)
        assert len({w["frame1 plane0"] for w in want}) == K, "the GOPs must differ"
        for delayed in (None,) + tuple(range(K)):
            got = threaded(rig, rig.crew, [(lambda S, g, order=order: decode(kept[order][g][0], order, net), [k])
                                           for k in range(K)], delayed, ms, f"decode_files {order}, delayed {delayed}")
            for k in range(K):
                _same(_as_bytes(got[k][0]), want[k], f"decode_gop_files ({order}), thread {k}, delayed thread {delayed}")
        eng = net.engine()
        out[order] = {"side_streams": len(eng.side_streams), "batch_streams": len(eng.batch_streams)}
        assert len(eng._llw) >= 1 and len(eng._dev_tab) >= 1 and eng.batch_streams
    # the temporal synthesis alone, on the tensors the encoder returned
    with torch.no_grad():
        want = [_as_bytes(synth(enc, enc_net)) for _, enc in kept["plane"]]
    torch.cuda.synchronize(rig.dev)
    for delayed in (None,) + tuple(range(K)):
        got = threaded(rig, rig.crew, [(lambda S, g: synth(kept["plane"][g][1], net), [k]) for k in range(K)], delayed,
                       rig.so.ENGINE_DELAY_MS["pairs"], f"decode_gop, delayed {delayed}")
        for k in range(K):
            _same(_as_bytes(got[k][0]), want[k], f"decode_gop, thread {k}, delayed thread {delayed}")
    return out


def case_two_models(rig, shared):
    """case 6: two models on one device, one per thread: A with plans on (it records, then replays), B with plans off
    throughout; both against their serial runs, both joined under a time limit (a gate that never opens fails here)"""
    ref = rig.model(plans=False)
    want = serial_encode(rig, ref, "pairs", range(4))
    a, b = rig.model(plans=True), rig.model(plans=False)
    nets, gops = (a, b), ((0, 1), (2, 3))
    crew = ht.Crew(2)                                        # the two threads stay: A's plans are keyed by its thread
    keys = ("pairs", "plans_off")
    counts = []
    try:
        for delayed in (None, 0, 1):
            folders = [[rig.folder(f"two_models_{'ab'[k]}_gop{g}") for g in gops[k]] for k in range(2)]

            def job(k):
                return lambda S, g: _harvest(_encode(nets[k], "pairs", rig.pictures(g), folders[k][gops[k].index(g)]))
            with Replays() as rp:
                got = threaded(rig, crew, [(job(k), list(gops[k])) for k in range(2)], delayed,
                               rig.so.ENGINE_DELAY_MS[keys[delayed or 0]], f"two_models, delayed {delayed}")
            counts.append(rp.n)
            for k in range(2):
                for u, g in enumerate(gops[k]):
                    _same(_as_bytes(got[k][u], folders[k][u]), want[g],
                          f"two models, model {'AB'[k]}, GOP {g}, delayed thread {delayed}")
            # A recorded during its first GOP (stream launches) and replays from then on; B never records
            assert a.engine().use_graphs and len(a.engine().host_threads) == 1, "model A lost its plans"
            assert rp.n == (3 if delayed is None else 6), f"model A replayed {rp.n} pairs (delayed thread {delayed})"
            assert not b.engine().pair_plans and not b.engine().use_graphs
    finally:
        if not crew.stuck:
            crew.close()
    return {"replays_of_model_a": counts}


def engine(group, scratch):
    rig = Rig(scratch)
    shared, out = {}, {}
    try:
        for name in GROUPS[group]:
            t0 = time.perf_counter()
            out[name] = globals()[f"case_{name}"](rig, shared)
            out[name]["seconds"] = round(time.perf_counter() - t0, 2)
            out[name]["runs"] = {k: v for k, v in rig.figures.items() if k.startswith(name) or
                                 (name == "decode_files" and k.startswith("decode_gop"))}
    finally:
        if not rig.crew.stuck:
            rig.crew.close()
    import torch
    torch.cuda.synchronize(rig.dev)
    return out


def main():
    mode = sys.argv[1]
    result = sys.argv[2] if mode == "abi" else sys.argv[3]
    t0 = time.perf_counter()
    try:
        out = abi() if mode == "abi" else engine(sys.argv[2], sys.argv[4])
        out.update(ok=True, total_seconds=round(time.perf_counter() - t0, 2))
    except Stuck as e:
        json.dump({"ok": False, "stuck": True, "error": str(e)}, open(result, "w"))
        sys.stdout.flush()
        os._exit(3)                                          # a thread is still inside the engine: nothing more on the GPU
    except BaseException as e:  # noqa: BLE001 - the parent reads the file
        out = {"ok": False, "error": f"{type(e).__name__}: {e}", "trace": traceback.format_exc()[-6000:]}
    json.dump(out, open(result, "w"))
    sys.exit(0 if out["ok"] else 1)


if __name__ == "__main__":
    main()
