"""The engine's hand-offs under delays (part 2): the codec at the suite's small configuration, coded once on
the default stream with nothing delayed (the baseline) and again on a stream of the test's own with the pictures uploaded
behind a bounded delay and, per run, one of the engine's own streams delayed in front of every pair.  Every file byte and
every returned tensor must be the baseline's: a missing wait, a copy on the wrong stream or a buffer handed on too early
gives another GOP's bytes, since the three GOPs differ in content.

Not collected by name: tests/test_gpu_stream_order_engine.py runs this module in fresh child processes that get eight
hardware queues, since the caller's stream needs a window against the default stream and EVERY stream of the engine, and
four queues cannot give it one.  A run whose caller's stream lacks one of those windows fails."""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

import stream_order as so
from helpers import frames, product_model

pytestmark = pytest.mark.gpu

W, H, GOP, Q = 132, 100, 4, 3                            # padded to 256x128
SEEDS = (41, 43, 47)                                     # three GOPs of different content: nine pairs


@pytest.fixture(scope="module")
def rig(cuda, tmp_path_factory):
    """one model, the pinned pictures, the candidate caller streams with their windows"""
    net, _ = product_model(1)
    eng = net.engine()
    eng.plan_context()                                   # the plan streams exist from here on
    pinned = [[[t.pin_memory() for t in f] for f in frames(W, H, GOP, seed=s)] for s in SEEDS]
    rig = {"net": net, "eng": eng, "pinned": pinned, "cands": candidates(cuda), "dev": cuda, "n": 0, "baseline": {},
           "times": {}, "tmp": tmp_path_factory.mktemp("stream_order")}
    caller_for(rig)
    yield rig
    print("\nhost milliseconds per GOP, (mode, delayed, GOP) -> runs:", rig["times"])


def candidates(dev):
    """eight fresh streams, each with the windows measured so far (filled in by caller_for)"""
    return [(torch.cuda.Stream(device=dev), {}) for _ in range(8)]


def caller_for(rig, unused=()):
    """The caller's stream: the first candidate with a window, both ways, against the default stream and every stream
    the engine owns by now (all but those named in `unused`, which the case never touches).  Fails, not skips, when no
    candidate qualifies."""
    need = {"default": torch.cuda.default_stream(rig["dev"])}
    need.update({k: v for k, v in rig["eng"].owned_streams().items() if not k.startswith(tuple(unused) or ("\0",))})
    for s, w in rig["cands"]:
        for name, o in need.items():
            if name not in w:
                w[name] = so.window(s, o) and so.window(o, s)
        if all(w[name] for name in need):
            if rig.get("said") != sorted(need):
                rig["said"] = sorted(need)
                print(f"\ncaller stream with windows against all of {sorted(need)}; candidates so far: "
                      f"{[sorted(n for n, ok in c.items() if not ok) for _, c in rig['cands'] if c]} lack these")
            return s
    raise AssertionError(f"no candidate stream has a window against all of {sorted(need)}: "
                         f"{[w for _, w in rig['cands']]}")


def _tensor_bytes(t):
    t = t.force() if hasattr(t, "force") else t
    return so._bytes(t)                                  # a copy on the current stream, then its synchronisation


def code(rig, mode, S=None, target=None, delayed=False, slow_coder_ms=0):
    """The three GOPs through `mode` (pairs | plans_off | batched | lazy | decoder; plans_off_multi and batched_multi: luma
    and chroma on the engine's two side streams, what PMCTF_MULTI_STREAM=1 selects) on stream S (None: the default one,
    nothing delayed).  delayed: the pictures of every GOP are uploaded behind a delay on S, and with an engine stream as
    `target` that stream is delayed in front of every pair (every GOP where the mode has no hook per pair).  The plans a
    mode records stay with the model: only the first run of "pairs" goes through stream launches and recordings.
    -> ({name: bytes} of every file and tensor, [folder per GOP]); rig["replays"]: plan replays of this run"""
    import time
    import warnings
    import pmctf_gop
    from pMCTF.hip import engine as engine_mod, pair_plan
    net, eng, dev = rig["net"], rig["eng"], rig["dev"]
    S = S or torch.cuda.default_stream(dev)
    from pMCTF.hip import ops
    base = mode.replace("_multi", "")
    ms = so.ENGINE_DELAY_MS[base] if delayed else 0.0
    before = (net.lazy_stages, eng.use_graphs, eng.multi_stream, eng.plan_timing, ops.CONV_PROBE)
    eng.use_graphs = base != "plans_off"
    eng.multi_stream = mode.endswith("_multi")
    net.lazy_stages = base == "lazy"
    if delayed and base == "pairs":
        eng.plan_timing = []                             # the plans' timing events are hand-off sites too
    if delayed and base == "plans_off":
        ops.CONV_PROBE = {"match": lambda conv, x, stride: True, "events": []}      # and the timing events around a conv
    rig["n"] += 1
    out, folders = {}, []

    def inject(*_):
        if ms and target not in (None, "caller"):
            so.delay(eng.owned_streams()[target], ms)
    orig_run, orig_replay, rig["replays"] = engine_mod.RangeCoderPool._run, pair_plan.PairPlan.run, 0

    def counted(self, *a, **k):
        rig["replays"] += 1
        return orig_replay(self, *a, **k)
    pair_plan.PairPlan.run = counted
    if slow_coder_ms:
        def slow(self, *a):
            time.sleep(slow_coder_ms / 1e3)              # the job reads its pinned buffers late
            return orig_run(self, *a)
        engine_mod.RangeCoderPool._run = slow
    try:
        with torch.cuda.stream(S), torch.no_grad(), warnings.catch_warnings():
            warnings.filterwarnings("error", message="pMCTF: recording the launch plan failed")
            for g, gop in enumerate(rig["pinned"]):
                folder = str(rig["tmp"] / f"run{rig['n']}_gop{g}")
                os.makedirs(folder)
                folders.append(folder)
                if ms:
                    so.delay(S, ms)
                pics = [[t.to(dev, non_blocking=True) for t in f] for f in gop]
                inject()
                t0 = time.perf_counter()
                if base == "batched":
                    enc = pmctf_gop.encode_gop_batched(net, pics, H, W, Q, folder)
                else:
                    enc = pmctf_gop.encode_gop(net, pics, H, W, Q, folder, skip_decoding=base != "decoder",
                                               on_pair=inject, store_only=base == "lazy")
                net.flush()
                rig["times"].setdefault((mode, bool(ms), g), []).append(round((time.perf_counter() - t0) * 1e3, 1))
                for i, fc in enumerate(enc["frames_coded"]):
                    for j, t in enumerate(fc):
                        if t is not None:
                            out[f"gop{g} frame{i} tensor{j}"] = _tensor_bytes(t)
                for i, r in enumerate(enc["results"]):
                    for k in ("mv_feature", "ref_mv_y"):
                        out[f"gop{g} pair{i} dpb {k}"] = _tensor_bytes(r["dpb"][k])
                out[f"gop{g} bits"] = repr((enc["bits"], enc["bits_mv"])).encode()
                for name in sorted(os.listdir(folder)):
                    out[f"gop{g} file {name}"] = open(os.path.join(folder, name), "rb").read()
    finally:
        engine_mod.RangeCoderPool._run, pair_plan.PairPlan.run = orig_run, orig_replay
        net.lazy_stages, eng.use_graphs, eng.multi_stream, eng.plan_timing, ops.CONV_PROBE = before
    torch.cuda.synchronize(dev)
    return out, folders


def baseline(rig, mode):
    if mode not in rig["baseline"]:
        rig["baseline"][mode] = code(rig, mode)          # "pairs": stream launches, and the plans are recorded
        again, _ = code(rig, mode)
        assert again == rig["baseline"][mode][0], f"{mode}: two undelayed runs differ"
        assert rig["replays"] == (3 * len(SEEDS) if mode == "pairs" else 0)
        files = [k for k in again if " file " in k]
        assert len(files) == len(SEEDS) * (3 * (GOP - 1) + 2)
        assert len({again[k] for k in files if k.endswith(" file 1.bin")}) == len(SEEDS), "the GOPs must differ"
    return rig["baseline"][mode]


def compare(got, want, what):
    assert sorted(got) == sorted(want), what
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{what}: {len(bad)} of {len(want)} files and tensors differ from the undelayed run: {bad[:8]}"


ENGINE_STREAMS = ("caller", "plan_luma", "plan_chroma", "motion", "side0", "side1")


@pytest.mark.parametrize("target", ENGINE_STREAMS)
def test_harness_loop_under_a_delay(rig, target):
    """case 1, the replays: encode_one_stage pair by pair through the recorded plans"""
    want, _ = baseline(rig, "pairs")
    got, _ = code(rig, "pairs", caller_for(rig), target, True)
    assert rig["replays"] == 3 * len(SEEDS)
    compare(got, want, f"harness loop, delay on {target}")


def test_harness_loop_recording_under_a_delay(rig, tmp_path):
    """case 1, a model of its own on the caller's stream: the pairs of GOP 0 by stream launches, each followed by the
    recording of its plan, GOPs 1 and 2 replayed; the pictures arrive behind a delay"""
    want, _ = baseline(rig, "pairs")
    net, _ = product_model(1)
    eng = net.engine()
    eng.plan_context()
    own = dict(rig, net=net, eng=eng, tmp=tmp_path, times={}, cands=candidates(rig["dev"]), said=None)
    got, _ = code(own, "pairs", caller_for(own), "caller", True)
    assert own["replays"] == 3 * (len(SEEDS) - 1)
    compare(got, want, "harness loop with recordings, delay on caller")


@pytest.mark.parametrize("target", ("caller", "motion", "side0", "side1"))
def test_harness_loop_without_plans_under_a_delay(rig, target):
    """case 2: the same by stream launches only"""
    want, _ = baseline(rig, "plans_off")
    compare(want, baseline(rig, "pairs")[0], "plans off against plans on, undelayed")
    got, _ = code(rig, "plans_off", caller_for(rig), target, True)
    compare(got, want, f"plans off, delay on {target}")


@pytest.mark.parametrize("target", ("caller", "motion", "side0"))
def test_stage_batched_with_overlap_under_a_delay(rig, target):
    """case 3: encode_stage_pairs, its motion chain on the engine's motion stream behind lt_event"""
    assert rig["eng"].motion_overlap
    want, _ = baseline(rig, "batched")
    got, _ = code(rig, "batched", caller_for(rig), target, True)
    compare(got, want, f"stage-batched, delay on {target}")


@pytest.mark.parametrize("target", ("caller", "side0", "side1"))
@pytest.mark.parametrize("mode", ("plans_off_multi", "batched_multi"))
def test_luma_and_chroma_on_the_side_streams_under_a_delay(rig, mode, target):
    """cases 2 and 3 with the two coders of a pair on the engine's side streams (PMCTF_MULTI_STREAM=1): the same files
    and tensors as the pair-by-pair run on one stream"""
    want, _ = baseline(rig, "pairs")
    got, _ = code(rig, mode, caller_for(rig), target, True)
    compare(got, want, f"{mode}, delay on {target}")


@pytest.mark.parametrize("target", ("caller", "motion"))
def test_deferred_mode_under_a_delay(rig, target):
    """case 4: lazy_stages, several pairs in flight"""
    want, _ = baseline(rig, "lazy")
    got, _ = code(rig, "lazy", caller_for(rig), target, True)
    compare(got, want, f"deferred mode, delay on {target}")


@pytest.mark.parametrize("target", ("caller", "side0", "side1"))
def test_decoder_in_the_loop_under_a_delay(rig, target):
    """case 5: skip_decoding=False: decompress_mv and _decompress_files inside every pair"""
    want, _ = baseline(rig, "decoder")
    got, _ = code(rig, "decoder", caller_for(rig), target, True)
    compare(got, want, f"decoder in the loop, delay on {target}")


DEC_GOP = 2                                              # four files per GOP: four side streams and two batch streams


@pytest.fixture(scope="module")
def dec_rig(cuda, tmp_path_factory):
    """Case 6 has a model and a process of its own: a GOP of four makes the engine open eight side streams, more than
    eight hardware queues can keep apart from the caller's.  Two GOPs of two pictures, coded here by stream launches in
    both LL orders (no plan streams come into being)."""
    import pmctf_gop
    net, _ = product_model(1)
    eng = net.engine()
    eng.use_graphs = False
    tmp = tmp_path_factory.mktemp("stream_order_decode")
    folders = {"plane": [], "position": []}
    with torch.no_grad():
        for order, skip in (("plane", True), ("position", False)):
            for s in SEEDS[:2]:
                folder = str(tmp / f"{order}_{s}")
                os.makedirs(folder)
                pmctf_gop.encode_gop(net, frames(W, H, DEC_GOP, device="cuda", seed=s), H, W, Q, folder, skip_decoding=skip)
                folders[order].append(folder)
        net.flush()
    torch.cuda.synchronize(cuda)
    return {"net": net, "eng": eng, "dev": cuda, "cands": candidates(cuda), "folders": folders, "baseline": {}}


class LatePool(ThreadPoolExecutor):
    """the pool of the finishing threads, every job entered 50 ms late"""

    def submit(self, fn, *a, **k):
        def late():
            time.sleep(0.05)
            return fn(*a, **k)
        return super().submit(late)


def _decode(rig, order, S=None, target=None, ms=0.0, late=False):
    import pmctf_gop
    net, eng, dev = rig["net"], rig["eng"], rig["dev"]
    S = S or torch.cuda.default_stream(dev)
    out = {}
    before = eng._batch_pool
    if late:
        workers = max(1, min(16, int(eng.decode_workers)))
        eng._batch_pool = (workers, LatePool(max_workers=workers))
    try:
        with torch.cuda.stream(S):
            for g, folder in enumerate(rig["folders"][order]):
                if ms:
                    so.delay(S, ms)
                    st = eng.owned_streams().get(target)
                    if st is not None:
                        so.delay(st, ms)
                dec = pmctf_gop.decode_gop_files(net, folder, DEC_GOP, H, W, Q, ll_order=order)
                for i, f in enumerate(dec["frames"]):
                    for j, t in enumerate(f[:2]):
                        out[f"gop{g} frame{i} plane{j}"] = _tensor_bytes(t)
    finally:
        if late:
            eng._batch_pool[1].shutdown(wait=True)
            eng._batch_pool = before
    torch.cuda.synchronize(dev)
    return out


@pytest.mark.parametrize("kind", ("caller", "batch", "side", "late host"))
@pytest.mark.parametrize("order", ("plane", "position"))
def test_gop_decode_under_a_delay(dec_rig, order, kind):
    """case 6: decode_gop_files in both LL orders: the caller's stream, every batch stream and every side stream the
    engine has made delayed in turn, and the finishing threads entered 50 ms late behind a delayed caller"""
    rig = dec_rig
    want = rig["baseline"].get(order)
    if want is None:
        want = rig["baseline"][order] = _decode(rig, order)
        assert _decode(rig, order) == want
        assert len({want[f"gop{g} frame1 plane0"] for g in range(2)}) == 2, "the GOPs must differ"
    streams = sorted(rig["eng"].owned_streams())
    assert [k for k in streams if k.startswith("side")] == [f"side{i}" for i in range(2 * DEC_GOP)]
    assert [k for k in streams if k.startswith("batch")], "the batched LL decode has run"
    S = caller_for(rig, unused=("motion",))              # decoding never touches the motion stream
    targets = [k for k in streams if k.startswith(kind)] if kind in ("batch", "side") else ["caller"]
    for target in targets:
        compare(_decode(rig, order, S, target, so.ENGINE_DELAY_MS["decode"], late=kind == "late host"), want,
                f"GOP decode ({order}), delay on {target}, {kind}")


@pytest.mark.parametrize("mode", ("pairs", "batched", "lazy"))
def test_slow_range_coder_under_a_delay(rig, mode):
    """case 7: every range-coder job reads its pinned buffers 50 ms late: two consecutive replays of one plan must not
    overwrite symbols the previous job still borrows"""
    want, _ = baseline(rig, mode)
    got, _ = code(rig, mode, caller_for(rig), "caller", True, slow_coder_ms=50)
    compare(got, want, f"{mode} with a slow range coder")


def _sequence(rig, tmp, name, S=None, ms=0.0):
    """case 8's run: eight pictures through encode_sequence (picture hashes on) and decode_sequence_checked"""
    import pmctf_gop
    import pmctf_synth
    net, dev = rig["net"], rig["dev"]
    S = S or torch.cuda.default_stream(dev)
    src, bins, yuv = str(tmp / "src.yuv"), str(tmp / name), str(tmp / f"{name}.yuv")
    if not os.path.exists(src):
        pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(W, H, 2 * GOP, seed=5))
    os.makedirs(bins)
    with torch.cuda.stream(S):
        if ms:
            so.delay(S, ms)                              # the ingest of the first GOP waits behind it
        pmctf_gop.encode_sequence(net, src, W, H, 2 * GOP, GOP, Q, bins, "cuda", keep_gops=True, picture_hash="f32")
        if ms:
            so.delay(S, ms)
        res = pmctf_gop.decode_sequence_checked(net, bins, yuv, "cuda", verify=True)
    torch.cuda.synchronize(dev)
    out = {"yuv": open(yuv, "rb").read(), "verdict": repr((res["hash_mismatches"], res["verified"], res["frames"])).encode()}
    for d, _, fs in os.walk(bins):
        for f in fs:
            if f != "sequence.json":                     # the header's fields are the arguments above
                out[os.path.relpath(os.path.join(d, f), bins)] = open(os.path.join(d, f), "rb").read()
    return out


def test_whole_sequence_under_a_delay(rig, tmp_path):
    """case 8: files, the decoded .yuv and the hash verdict of a sequence coded and decoded on the caller's stream, the
    ingest behind a delay, equal those of the undelayed run on the default stream"""
    S = caller_for(rig)                                  # against every stream that can read the ingested pictures: the
    want = _sequence(rig, tmp_path, "plain")             # decoder's further side and batch streams come into being below,
    assert want["verdict"] == repr(([], 2 * GOP, [(H, W)] * (2 * GOP))).encode()      # and case 6 holds those
    assert len(want) == 2 + 1 + 2 * (3 * (GOP - 1) + 2), sorted(want)
    got = _sequence(rig, tmp_path, "delayed", S, so.MAX_DELAY_MS)
    compare(got, want, "whole sequence, delayed ingest")
