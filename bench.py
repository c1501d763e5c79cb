#!/usr/bin/env python3
"""bench.py — encoded 1080p frames/s of the pMCTF temporal-decomposition encode path on MI355X.

One "step" = one full GOP-16 encode of 1920x1080 4:2:0 frames at q_index=3, inputs already resident in HBM,
bitstreams written by the host range coder.

`value` times what the UNMODIFIED reference harness gets: pmctf_gop.encode_gop restates its loop statement for
statement (test_pMCTF_flex.py:196-258) — pMCTF.encode_one_stage once per frame pair, 15 pairs + the final L frame per
GOP, and after EVERY call the two f-strings the script prints, which look at that pair's bit counts (:240, :248).
Every pair is therefore finished (files written, sizes known) before the next call starts.  The model is in its default
mode: finished tensors and Python floats per call; from the second pair of a configuration on it replays captured
launch plans (HIP graphs, luma / chroma coders of the pair on two streams, pMCTF.hip.pair_plan).
A plain run sets up, warms up, times exactly --steps steps, writes the last step's outputs when --dump-outputs DIR is
given (dump_outputs) and prints the line: `value`, `ms_per_step`, bpp and the configuration.  Everything below is
measured and checked only with --full.
With --full, after the timed region, rank 0 also measures (auxiliary figures, never `value`):
  * `roofline` / `stream_launches_single_stream` — the same loop with the plans off: plain stream launches on ONE
                          stream, the dominant convolution bracketed by HIP events on that stream (with the plans on,
                          luma and chroma kernels share the GPU, which per-kernel events cannot separate);
  * `cpu_baseline`      — the oracle's ATen-CPU restatement timed on one full-size 1080p pair on the host cores;
and, while the wall-clock budget for auxiliary legs (--aux_budget_s) lasts:
  * `deferred_store_only` — a caller that only STORES the results (the harness loop WITHOUT its two prints) with the
                          model's opt-in deferral: the pairs of a temporal stage coded as one batch;
  * `stage_batched`     — all pairs of a temporal stage in one call (pMCTF.encode_stage_pairs);
  * `cross_gop_batched` — the same with stage s of K closed GOPs in one call (pmctf_gop.encode_gops_batched);
  * `decode_pair`       — one 1080p pair with skip_decoding=False: the real decoder's time;
  * `hbm_kernels`       — the bandwidth-bound kernels of the path (warp, lifting add, depthwise, few-channel convolutions,
                          resampling) on their 1080p shapes: algorithmic GB/s against the 8 TB/s HBM peak;
  * `aux_profiles`      — the reduced-precision arithmetic profiles (no parity claim).
N GPUs encode N independent GOPs (closed GOPs are independent units: no data-path collective; weak scaling) — that is
`value`; with N > 1 the same ranks then time the north-star layout as `pair_sharded`: ONE GOP, the pairs of each
temporal stage spread over the ranks, motion context relayed rank to rank, one all-gather of the subband tree per
stage over RCCL (strong scaling), alone and — from three ranks on — with max(2, N/2) closed GOPs in flight.
That block (--full only) runs after the timed region and its roofline pass and under a watchdog
(--pair_shard_timeout_s): a rank that dies or a collective that never completes costs the block, never the line.
Prints ONE JSON line on rank 0.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import atexit
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))

# work of one 1080p pair in GMAC: coded frame 10 186, SpyNet 707, MV codec 163, temporal P+U 32.5
_W_FRAME, _W_MOTION = 10186.0, 707.0 + 163.0 + 32.5
PEAK_F32_MFMA = 157.3          # TFLOP/s, MI355X peak FP32 (matrix)
DUMP_BYTES = 64_000_000        # --dump-outputs writes at most this much


def scratch_dir(prefix):
    """a folder for the bitstreams of the run, removed when the process exits"""
    d = tempfile.mkdtemp(prefix=prefix)
    atexit.register(shutil.rmtree, d, True)
    return d


def dump_outputs(folder, enc, bin_folder):
    """--dump-outputs DIR: what a caller of the timed path received from its last step, one float32 / float64 .npy per
    array: bits and motion bits per frame, the coded tree of every frame (frames_coded of pmctf_gop.encode_gop: luma and
    chroma subbands, decoded motion) and the bitstream files of that step (their sizes, and their bytes concatenated in
    name order).  Frames and weights come from fixed seeds, so two builds run with the same arguments can be compared
    file for file.  An array larger than its share of DUMP_BYTES is written as a fixed sample of its flattened elements
    (seeded by its name: the same indices in every run)."""
    import zlib
    import numpy as np
    arrays = {"bits": np.asarray(enc["bits"], dtype=np.float64), "bits_mv": np.asarray(enc["bits_mv"], dtype=np.float64)}
    for i, coded in enumerate(enc["frames_coded"]):
        for part, t in zip(("y", "c", "mv"), coded):
            if t is not None:
                arrays[f"frame{i:02d}_{part}"] = t.detach().float().cpu().numpy()
    blobs = []
    for n in sorted(os.listdir(bin_folder)):
        with open(os.path.join(bin_folder, n), "rb") as f:
            blobs.append(f.read())
    arrays["bitstream_sizes"] = np.array([len(b) for b in blobs], dtype=np.float64)
    arrays["bitstream_bytes"] = np.frombuffer(b"".join(blobs), dtype=np.uint8).astype(np.float32)
    share = (DUMP_BYTES - 4096 * len(arrays)) // len(arrays)     # bytes per array; an .npy header takes less than 4 KB
    os.makedirs(folder, exist_ok=True)
    for name, a in arrays.items():
        keep = share // a.itemsize
        if a.size > keep:
            idx = np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, keep, replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(folder, name + ".npy"), a)


def cpu_baseline(width, height, gop, q_index):
    """The oracle's restatement with the ATen CPU ops the reference itself calls (kind "port"), timed on the host cores
    on a bounded sample of the SAME workload: one full-size H pair of the 1080p sequence (stage 0, no L).  The pair that
    also codes L does one more coded frame: t_HL = t_H * (2*10186 + 902.5) / (10186 + 902.5) by the conv work of
    BASELINE.md §3; GOP time = (gop-2)*t_H + t_HL."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import pmctf_synth
    from pmctf_oracle.model import Oracle
    from pMCTF.models.video.pMCTF_L import pMCTF
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(16, avail)))       # a 1-GPU box owns a 16-CPU share of the host
    net = pMCTF(num_me_stages=1)
    sd = pmctf_synth.synth_state_dict(net.state_dict(), seed=0)
    orc = Oracle(sd, 1, "torch")
    dpb = {"mv_feature": None, "ref_mv_y": None}
    fr = [list(pmctf_synth.frames_to_tensors(f)) for f in pmctf_synth.synth_yuv420(width, height, 2)]
    with torch.no_grad():
        t0 = time.time()
        orc.encode_one_stage(fr[0], fr[1], False, dpb, pic_width=width, pic_height=height, q_index=q_index)
        t_h = time.time() - t0
    ratio = (2 * _W_FRAME + _W_MOTION) / (_W_FRAME + _W_MOTION)
    t_gop = (gop - 2) * t_h + ratio * t_h
    return {"value": gop / t_gop, "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle (ATen CPU ops, as the reference's CPU path) on ONE full-size {width}x{height} H pair: "
                      f"t_H = {t_h:.1f} s; GOP = {gop - 2}*t_H + t_HL with t_HL = {ratio:.3f}*t_H (conv work ratio)",
            "t_h_pair_s": t_h}


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N ranks through torch.distributed.run as a CHILD process
    (nothing has touched the GPU in this process yet) and exit with its status."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def roofline_of(events, kernels, traffic, probe_pass):
    """dominant-kernel roofline from HIP events recorded on the launch stream; `kernels`: what the C side launched for
    those convolutions (pmctf_conv2d_last_launch), with counts"""
    durs = [e0.elapsed_time(e1) * 1e-3 for e0, e1, _ in events]
    flops_all = [f for _, _, f in events]
    # launches of this convolution can differ in batch size: rate = total FLOP / total time
    achieved = sum(flops_all) / sum(durs) / 1e12 if durs else None     # None: no launch of that shape (small frames)
    return {"bound": "mfma", "kernel": "3x3 112->112 convolution on 576x960 luma subband planes, f32 MFMA 16x16x4; launched as: "
                                       + "; ".join(f"{n}x {k}" for k, n in sorted(kernels.items(), key=lambda kv: -kv[1])),
            "achieved": achieved, "peak": PEAK_F32_MFMA, "unit": "TFLOP/s",
            "frac": None if achieved is None else achieved / PEAK_F32_MFMA, "launches": len(durs),
            "avg_launch_ms": sum(durs) / len(durs) * 1e3 if durs else None,
            "flops_per_launch": sum(flops_all) / len(flops_all) if durs else 0.0, "traffic": traffic,
            "traffic_unit": "HBM bytes per 576x960x112 plane of the convolution (rocprofv3 --pmc passes committed under "
                            "profiles/: FETCH_SIZE x2 + WRITE_SIZE); algorithmic 495.9e6 B per plane; a launch over N "
                            "planes moves N times that",
            "probe_pass": probe_pass}


def parity_sweep():
    """what the strict 1080p tests measured against the real reference's digests for every rate point (data:
    tests/golden/headline_pins.json, written from a GPU run of tests/test_gpu_engine.py)"""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "headline_pins.json")) as f:
            pins = json.load(f)
    except (OSError, ValueError):
        return None
    out = {}
    for k, p in sorted(pins.items()):
        out[k] = {"frames_with_bit_delta": sum(1 for d in p["dbits"] if d), "bit_deltas": [d for d in p["dbits"] if d],
                  "max_abs_dpsnr_db": p["psnr_err"], "files_identical": p["same"], "files": p["same"] + p["diff"],
                  "meets_bar": not any(p["dbits"]) and p["psnr_err"] < 1e-4}
    return out


def main():
    t_process = time.time()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gop", type=int, default=16)
    ap.add_argument("--q_index", type=int, default=3)
    ap.add_argument("--no_cpu_baseline", action="store_true")
    ap.add_argument("--no_aux", action="store_true", help="skip the auxiliary schedules measured after the timed region")
    ap.add_argument("--aux_budget_s", type=float, default=240.0,
                    help="wall-clock budget of the OPTIONAL legs after the timed region (roofline pass and cpu_baseline are "
                         "not optional); a leg only starts while the budget lasts")
    ap.add_argument("--schedule", choices=("pairs", "stages"), default="pairs",
                    help="what `value` times.  pairs (default): the reference harness's loop, one encode_one_stage call per "
                         "frame pair, bit counts looked at after every call.  stages: the pairs of each temporal stage as "
                         "one batch (encode_stage_pairs): same files and bits, larger launches.")
    ap.add_argument("--aux_precisions", default="f32-chain,bf16x3,bf16x2,bf16",
                    help="auxiliary profiles measured after the exact run ('' to skip): f32-chain (entropy-parameter networks "
                         "as plain chains: faster, a CDF row off now and then) and the reduced-precision ones")
    ap.add_argument("--cross_gops", type=int, default=4, help="K of the auxiliary cross-GOP stage-batched figure")
    ap.add_argument("--inflight", type=int, default=1,
                    help="closed GOPs coded concurrently on this GPU (one host thread + HIP stream each; a step is then "
                         "`inflight` GOPs).")
    ap.add_argument("--shard", choices=("gops", "pairs"), default="gops",
                    help="what `value` times with N > 1.  gops: every rank codes its own GOP (weak scaling, no data-path "
                         "collective; the pair-sharded layout is then timed as the `pair_sharded` block).  pairs: ONE GOP, "
                         "the pairs of each temporal stage spread over the ranks (strong scaling).")
    ap.add_argument("--pair_shard_timeout_s", type=float, default=240.0,
                    help="watchdog of the `pair_sharded` block: print the line without it when it has not finished by then")
    ap.add_argument("--pair_shard_steps", type=int, default=2, help="steps of the `pair_sharded` block (N > 1; 0 to skip)")
    ap.add_argument("--overlap_gops", type=int, default=0,
                    help="closed GOPs in flight in the `pair_sharded` block's overlapped variant (SURVEY 8e)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step to DIR/<name>.npy (rank 0; dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="after the line's own figures, also measure and check everything else: PSNR and parity against "
                         "the reference's digests, roofline pass, pair_sharded block, cpu_baseline, the auxiliary legs")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PMCTF_DIST_BACKEND", "nccl")     # "nccl" = RCCL over xGMI on the 8-GPU node
        if os.environ.get("PMCTF_BENCH_SINGLE_DEVICE"):               # rehearsal of the N>1 path on a 1-GPU box
            local_rank = 0
        kw = {"device_id": torch.device("cuda", local_rank)} if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import pmctf_gop
    import pmctf_synth
    from pMCTF.hip import ops
    from pMCTF.models.video.pMCTF_L import pMCTF

    stages = 1
    while 2 ** stages < args.gop:
        stages += 1
    net = pMCTF(num_me_stages=min(4, stages)).eval()
    net.load_state_dict(pmctf_synth.synth_state_dict(net.state_dict(), seed=0), strict=True)
    net = net.to(dev)
    net.update(force=True)

    if args.inflight > 1:
        # several host threads drive the engine: launch plans are for one (a stream capture cannot coexist with another
        # thread's device synchronisations), so this mode uses stream launches throughout
        net.engine().use_graphs = False
    W, H = args.width, args.height

    def gop_frames(seed):
        return [list(pmctf_synth.frames_to_tensors(f, device=dev)) for f in pmctf_synth.synth_yuv420(W, H, args.gop, seed=seed)]

    # every rank codes its own GOP (different frames of the synthetic sequence)
    frames = gop_frames(1234 + (rank if args.shard == "gops" else 0))
    PH, PW = frames[0][0].shape[2], frames[0][0].shape[3]
    sub_h, sub_w = PH // 2, PW // 2

    def dominant(conv, x, stride):   # ContextResidual 3x3 112->112 on a level-0 luma subband (full-resolution form)
        return stride == 1 and (not conv.small) and conv.Cin == 112 and conv.Cout == 112 and conv.KH == 3 and \
            x.shape[1] == sub_h and x.shape[2] == sub_w

    tmp = scratch_dir(f"pmctf_bench_r{rank}_")
    last = {}
    extra = []      # --inflight > 1: further GOPs of the synthetic sequence, each with its own stream and output folder
    for k in range(1, args.inflight):
        extra.append((gop_frames(1234 + rank + 1000 * k), torch.cuda.Stream(device=dev),
                      scratch_dir(f"pmctf_bench_r{rank}_g{k}_")))

    def code_extra(fr, stream, folder):
        torch.cuda.set_device(dev)
        with torch.no_grad(), torch.cuda.stream(stream):
            (pmctf_gop.encode_gop_batched if args.schedule == "stages" else pmctf_gop.encode_gop)(
                net, fr, H, W, args.q_index, folder)
        stream.synchronize()

    def step_main():
        if args.shard == "pairs" and world > 1:
            import pmctf_dist
            enc = pmctf_dist.encode_gop_pair_sharded(net, frames, H, W, args.q_index, tmp, rank, world, dist)
        elif args.schedule == "stages":
            enc = pmctf_gop.encode_gop_batched(net, frames, H, W, args.q_index, tmp)
        else:
            enc = pmctf_gop.encode_gop(net, frames, H, W, args.q_index, tmp)
        last["enc"] = enc

    def step():
        import threading
        workers = [threading.Thread(target=code_extra, args=e) for e in extra]
        for t in workers:
            t.start()
        step_main()
        for t in workers:
            t.join()

    def sync(collective=True):
        torch.cuda.synchronize()
        if dist is not None and collective:
            dist.barrier()

    def timed(fn, steps, warmup, probe_kernels=False, collective=True):
        """W untimed steps, then exactly K steps bracketed by barrier + synchronize; with probe_kernels, convolutions of
        the dominant shape that go through stream launches inside the timed region are bracketed by HIP events on the
        launch stream"""
        for _ in range(warmup):
            fn()
        sync(collective)
        probe = {"match": dominant, "events": [], "kernels": {}} if probe_kernels else None
        ops.CONV_PROBE = probe
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync(collective)
        elapsed = time.perf_counter() - t0
        ops.CONV_PROBE = None
        return elapsed, probe

    with torch.no_grad():
        elapsed, _ = timed(step, args.steps, args.warmup)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    frames_total = args.gop * args.steps * (world if args.shard == "gops" else 1) * args.inflight
    value = frames_total / elapsed
    eng = net.engine()
    plans_on = eng.use_graphs and not net.lazy_stages
    sched_text = {"pairs": "the reference harness's loop (test_pMCTF_flex.py:196-258): encode_one_stage pair by pair, the bit "
                           "counts of every pair looked at (its two f-strings, :240,:248) before the next call"
                           + ("; each call replays a captured launch plan (HIP graphs), luma / chroma coders on two streams"
                              if plans_on else "; stream launches") +
                           ("; results DEFERRED (PMCTF_LAZY=1)" if net.lazy_stages else ""),
                  "stages": "all pairs of a temporal stage as one batch (encode_stage_pairs)"}

    if rank == 0:
        enc = last["enc"]
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, enc, tmp)
        headline = (W, H, args.gop, args.q_index) == (1920, 1080, 16, 3)
        out = {
            "metric": "encoded 1080p frames/sec (GOP=16, q_index=3)" if headline
            else f"encoded {W}x{H} frames/sec (GOP={args.gop}, q_index={args.q_index})", "value": value, "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak" if args.shard == "gops" else "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{W}x{H} 4:2:0 GOP-{args.gop} q_index={args.q_index} full pMCTF encode "
                                   f"(write_stream, skip_decoding), num_me_stages={net.num_me_stages}",
                       "schedule": "pairs of each temporal stage spread over the ranks (encode_one_stage per pair, motion "
                                   "context relayed rank to rank, one all-gather per stage)"
                       if (args.shard == "pairs" and world > 1) else sched_text[args.schedule],
                       "frames_per_step": args.gop * args.inflight, "gops_in_flight_per_gpu": args.inflight,
                       "parallelism": f"gop-dp{world}" if args.shard == "gops" else f"pair-shard{world}",
                       "weights": "deterministic synthetic (pmctf_synth seed 0)"},
            "bpp": sum(enc["bits"]) / (args.gop * W * H),
        }
    if not args.full:
        if rank == 0:
            out["bench_wall_s"] = time.time() - t_process
            print(json.dumps(out), flush=True)
        leave_group(dist)
        return

    if rank == 0:
        rec = pmctf_gop.decode_gop(net, [list(f) for f in enc["frames_coded"]])
        ps = pmctf_gop.gop_psnr(rec, frames, H, W)
        out["psnr_yuv"] = sum(p["yuv"] for p in ps) / len(ps)
        # "+ bpp/PSNR parity vs CPU ref" of BASELINE's metric: rank 0 codes exactly the sequence the real reference was
        # run on (tools/make_golden.py --width 1920 --height 1080 --gop_only --gop 16 --me_stages 4 [--q_index q]);
        # compare with the digests of that run (data, tests/golden/).
        qs = "" if args.q_index == 3 else f"_q{args.q_index}"
        fix = os.path.join(ROOT, "tests", "golden",
                           f"reference_{W}x{H}_gop{args.gop}_me{net.num_me_stages}{qs}_digest.npz")
        if os.path.exists(fix):
            import numpy as np
            g = np.load(fix)
            out["parity_vs_reference_cpu"] = {
                "bits_per_frame_identical": enc["bits"] == g["gop.bits"].tolist(),
                "bpp_reference": float(g["gop.bits"].sum()) / (args.gop * W * H),
                "psnr_yuv_reference": float(g["gop.psnr_yuv"].mean()),
                "psnr_max_abs_err_db": float(max(abs(p["yuv"] - r) for p, r in zip(ps, g["gop.psnr_yuv"].tolist()))),
            }
        if headline:
            out["parity_sweep"] = parity_sweep()
        del rec
        traffic = None      # HBM bytes per plane of this kernel from the committed rocprofv3 --pmc passes (profiles/)
        for name in ("round4_dominant_kernel.json", "round3_dominant_kernel.json", "round2_dominant_kernel.json"):
            try:
                with open(os.path.join(ROOT, "profiles", name)) as f:
                    traffic = json.load(f)["traffic_bytes_per_launch"]
                break
            except (OSError, KeyError, ValueError):
                pass

        def leg(name, fn):
            """An auxiliary figure must never cost the headline line: a failing leg is recorded and skipped."""
            try:
                with torch.no_grad():
                    fn()
            except Exception as e:  # noqa: BLE001
                out.setdefault("aux_errors", {})[name] = f"{type(e).__name__}: {e}"[:300]

        aux_steps = max(1, min(args.steps, 3))
        single = world == 1 and args.inflight == 1

        # ---- not optional: the roofline pass (plans off, one stream: per-kernel events mean something) -------------------
        def roofline_pass():
            keep = eng.use_graphs
            eng.use_graphs = False
            try:
                gop_alone = lambda: last.__setitem__("enc", pmctf_gop.encode_gop(net, frames, H, W, args.q_index, tmp))
                t_s, pr = timed(gop_alone if world > 1 else step_main, aux_steps, 0, probe_kernels=True, collective=False)
            finally:
                eng.use_graphs = keep
            out["roofline"] = roofline_of(
                pr["events"], pr["kernels"], traffic,
                "separate pass of the same GOPs through stream launches on ONE stream, right after the timed region: in the "
                "timed region the launches are replayed from HIP graphs with luma and chroma kernels sharing the GPU, which "
                "per-kernel events cannot separate" if plans_on and args.schedule == "pairs" else
                "the timed schedule, stream launches")
            out["stream_launches_single_stream"] = {
                "value": args.gop * aux_steps / t_s, "unit": "frames/s", "ms_per_step": t_s / aux_steps * 1e3, "steps": aux_steps,
                "schedule": "the harness loop, every launch issued from the host on one stream (captured launch plans off)",
                "bits_identical_to_headline": last["enc"]["bits"] == enc["bits"]}
        if world == 1 or rank == 0:
            leg("roofline", roofline_pass)
        if "roofline" not in out:
            out["roofline"] = roofline_of([], {}, traffic, "failed")
        if headline and args.schedule == "pairs":
            # every convolution of the timed region against the same roof: 323.6 TFLOP per 1080p GOP-16 as this build
            # computes it (profiles/round3_conv_census_pairs.txt: every conv launch of one GOP, 2 FLOP per MAC; the
            # reference's own count is 353 TFLOP, the difference is the exact quarter-resolution evaluation of DESIGN §5)
            e2e = 323.6e12 * frames_total / args.gop / elapsed / 1e12
            out["roofline"]["end_to_end_timed_region"] = {
                "achieved": e2e, "unit": "TFLOP/s", "frac": e2e / (PEAK_F32_MFMA * world),
                "note": "all convolution FLOPs of the timed steps / their wall time (motion estimation, codecs, lifting, "
                        "entropy networks, post-processing; elementwise work and the host range coder included in the time)"}


    # ---- the north-star multi-GPU layout over the same ranks (N > 1): pairs of ONE GOP spread over the GPUs
    pair_sharded = None
    if world > 1 and args.shard == "gops" and args.pair_shard_steps > 0:
        # A rank that dies or a collective that never completes must not cost the line the driver reads: when the block
        # has not finished after --pair_shard_timeout_s, rank 0 prints what it has (the timed region and its roofline are
        # done by now) and every rank leaves without waiting for the others.
        import threading

        headline_line = dict(out) if rank == 0 else {}      # snapshot: the main thread keeps filling `out` while the timer runs

        def bail():
            # the line survives (the timed region and its roofline are done), the STATUS does not: a hung collective or
            # a dead rank must never read as success to the launcher
            if rank == 0:
                line = dict(headline_line)
                line["pair_sharded"] = {"error": f"no result within {args.pair_shard_timeout_s} s (watchdog): a rank "
                                                 f"failed or a collective did not complete"}
                line["bench_wall_s"] = time.time() - t_process
                print(json.dumps(line), flush=True)
            os._exit(3)
        watchdog = threading.Timer(args.pair_shard_timeout_s, bail)
        watchdog.daemon = True
        watchdog.start()
        import pmctf_dist
        frames0 = frames if rank == 0 else gop_frames(1234)       # every rank reads the same GOP (rank 0's)
        stats = {}

        def sharded():
            last["ps"] = pmctf_dist.encode_gop_pair_sharded(net, frames0, H, W, args.q_index, tmp, rank, world, dist,
                                                            stats=stats)
        blocks = {}
        try:
            with torch.no_grad():
                t_ps, _ = timed(sharded, args.pair_shard_steps, 1)
            tt = torch.tensor([t_ps], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            t_ps = float(tt.item())
            pair_sharded = {"value": args.gop * args.pair_shard_steps / t_ps, "unit": "frames/s", "scaling": "strong",
                            "ms_per_step": t_ps / args.pair_shard_steps * 1e3, "steps": args.pair_shard_steps,
                            "speedup_vs_one_gpu_coding_this_gop": (elapsed / args.steps) / (t_ps / args.pair_shard_steps),
                            "gather_bytes_per_stage": stats.get("gather_bytes_per_stage"),
                            "relay_hops": stats.get("relay_hops"), "relay_bytes_per_hop": stats.get("relay_bytes_per_hop"),
                            "collective": "all_gather_into_tensor (RCCL)" if dist.get_backend() == "nccl" else "all_gather (gloo)",
                            "schedule": "ONE GOP: pair k of a temporal stage on rank k mod N, motion context relayed rank to "
                                        "rank, one all-gather of the subband tree per stage; a stage with at most half as "
                                        "many pairs as ranks is shared in PARTS (motion + luma coders / chroma coders, in the "
                                        "last stage H and L coders on separate ranks) and reassembled by broadcasts of the "
                                        "live tensors only (pmctf_dist.pair_parts)",
                            "bits_identical_to_rank0_gop": (last["ps"]["bits"] == last["enc"]["bits"]) if rank == 0 else None}
            # closed GOPs in flight: 0 = as many as keep every rank busy in every stage (N / 2: the late stages of a
            # GOP-16 have 2 and 1 pairs), at least 2; DESIGN §7 has the expected critical paths
            G2 = args.overlap_gops if args.overlap_gops > 0 else max(2, world // 2)
            if G2 > 1 and world >= 3:     # with two ranks the GOPs would be coded one after the other
                gops = [frames0] + [gop_frames(1234 + 1000 * k) for k in range(1, G2)]
                folders = [tmp] + [scratch_dir(f"pmctf_bench_r{rank}_o{k}_") for k in range(1, G2)]

                def overlapped():
                    last["po"] = pmctf_dist.encode_gops_pair_sharded_overlapped(net, gops, H, W, args.q_index, folders,
                                                                                rank, world, dist)
                with torch.no_grad():
                    t_po, _ = timed(overlapped, max(1, args.pair_shard_steps // 2), 1)
                tt = torch.tensor([t_po], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                n_po = max(1, args.pair_shard_steps // 2)
                pair_sharded["overlapped_gops"] = {
                    "gops_in_flight": G2, "value": G2 * args.gop * n_po / float(tt.item()), "unit": "frames/s",
                    "ms_per_step": float(tt.item()) / n_po * 1e3, "steps": n_po,
                    "schedule": f"{G2} closed GOPs interleaved: ranks idle in the late stages of one GOP code the early stages "
                                f"of the next (SURVEY 8e)",
                    "bits_identical_to_rank0_gop": (last["po"][0]["bits"] == last["enc"]["bits"]) if rank == 0 else None}
        except Exception as e:  # noqa: BLE001 - an auxiliary block must never cost the headline line
            pair_sharded = {"error": f"{type(e).__name__}: {e}"[:300]}
        watchdog.cancel()

    if rank == 0:
        if pair_sharded is not None:
            out["pair_sharded"] = pair_sharded
        # ---- not optional: the CPU baseline -------------------------------------------------------------------------------
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(W, H, args.gop, args.q_index)
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": 0, "kind": "port", "sample": "failed",
                                       "error": f"{type(e).__name__}: {e}"[:300]}

        # ---- optional legs, while the budget lasts ------------------------------------------------------------------------
        t_aux = time.time()
        skipped = []

        def optional(name, fn):
            if time.time() - t_aux > args.aux_budget_s:
                skipped.append(name)
                return
            leg(name, fn)

        aux = single and not args.no_aux
        if aux and args.schedule == "pairs" and not net.lazy_stages:
            def deferred():
                net.lazy_stages = True
                try:
                    def run():
                        last["enc"] = pmctf_gop.encode_gop(net, frames, H, W, args.q_index, tmp, store_only=True)
                    t_d, _ = timed(run, aux_steps, 1)
                finally:
                    net.lazy_stages = False
                out["deferred_store_only"] = {
                    "value": args.gop * aux_steps / t_d, "unit": "frames/s", "ms_per_step": t_d / aux_steps * 1e3,
                    "steps": aux_steps,
                    "schedule": "the harness loop WITHOUT its two per-pair prints (a caller that only stores the results), "
                                "model with lazy_stages=True: the pairs of a temporal stage coded as one batch when the next "
                                "stage needs them (pMCTF.hip.deferred)",
                    "bits_identical_to_headline": last["enc"]["bits"] == enc["bits"]}
            optional("deferred_store_only", deferred)
        if aux and args.schedule == "pairs":
            def stage_batched():
                def batched():
                    last["enc"] = pmctf_gop.encode_gop_batched(net, frames, H, W, args.q_index, tmp)
                t_b, pr = timed(batched, aux_steps, 1, probe_kernels=True)
                out["stage_batched"] = {
                    "value": args.gop * aux_steps / t_b, "unit": "frames/s", "ms_per_step": t_b / aux_steps * 1e3,
                    "steps": aux_steps, "schedule": sched_text["stages"],
                    "bits_identical_to_headline": last["enc"]["bits"] == enc["bits"],
                    "roofline": roofline_of(pr["events"], pr["kernels"], traffic, "this leg's own timed region (stream launches)")}
            optional("stage_batched", stage_batched)
        K = args.cross_gops
        if aux and K > 1 and hasattr(pmctf_gop, "encode_gops_batched"):
            def cross_gop():
                gops = [frames] + [gop_frames(1234 + 1000 * k) for k in range(1, K)]
                folders = [tmp] + [scratch_dir(f"pmctf_bench_x{k}_") for k in range(1, K)]

                def cross():
                    last["encs"] = pmctf_gop.encode_gops_batched(net, gops, H, W, args.q_index, folders)
                k_steps = max(1, min(args.steps, 2))
                try:
                    t_x, pr = timed(cross, k_steps, 1, probe_kernels=True)
                    out["cross_gop_batched"] = {
                        "value": K * args.gop * k_steps / t_x, "unit": "frames/s", "ms_per_step": t_x / k_steps * 1e3,
                        "steps": k_steps, "gops_per_step": K, "frames_per_step": K * args.gop,
                        "schedule": f"stage s of {K} closed GOPs as one batch (pmctf_gop.encode_gops_batched)",
                        "bits_identical_to_headline": last["encs"][0]["bits"] == enc["bits"],
                        "roofline": roofline_of(pr["events"], pr["kernels"], traffic, "this leg's own timed region (stream launches)")}
                finally:
                    last.pop("encs", None)
            optional("cross_gop_batched", cross_gop)
        if aux:
            def decode_pair():
                # the real decoder (skip_decoding=False, the harness's default: test_pMCTF_flex.py:53): one H pair and the
                # pair that also codes L, decoded from the files just written (pMCTF_L.py:594-612)
                dpb0 = {"mv_feature": None, "ref_mv_y": None}
                res = {}
                for name, code_lt in (("h_pair", False), ("h_and_l_pair", True)):
                    ts = []
                    for _ in range(2):
                        r = net.encode_one_stage(frames[0], frames[1], code_lt, dpb0, output_path=os.path.join(tmp, "1.bin"),
                                                 pic_width=W, pic_height=H, skip_decoding=False, stage_idx=0,
                                                 q_index=args.q_index)
                        ts.append(r["decoding_time"])
                    res[name] = {"decoding_time_s": min(ts), "encoding_time_s": r["encoding_time"]}
                out["decode_pair"] = dict(res, unit="s per 1080p pair (motion + luma + chroma streams, files read back)",
                                          schedule="encode_one_stage(skip_decoding=False): decompress_mv + decompress_one_stage "
                                                   "of luma and chroma; the sequential LL subband decodes row by row (per row: the row-above part of every chain on "
                                                   "all CUs, then one sequential workgroup), the motion stream under it")
            optional("decode_pair", decode_pair)

        if aux and args.aux_precisions:
            # AUXILIARY arithmetic profiles (second conv variant): the dense 3x3 convolutions on bf16 MFMA
            # with operands split into 3 / 2 / 1 planes.  Reported beside the exact figure, never instead of it, with what
            # they cost in fidelity against the real reference's digests; dtype of the headline stays f32.
            import numpy as np
            out["aux_profiles"] = {}
            ref_bits = ref_psnr = None
            if os.path.exists(fix):
                g = np.load(fix)
                ref_bits, ref_psnr = g["gop.bits"], g["gop.psnr_yuv"]

            def profile(prec):
                net.precision = prec
                k_p = max(1, min(args.steps, 2))
                t_p, _ = timed(step_main, k_p, 1)
                e_p = last["enc"]

                def batched():
                    last["enc_b"] = pmctf_gop.encode_gop_batched(net, frames, H, W, args.q_index, tmp)
                t_pb, _ = timed(batched, k_p, 1)
                ps_p = pmctf_gop.gop_psnr(pmctf_gop.decode_gop(net, [list(f) for f in e_p["frames_coded"]]), frames, H, W)
                blk = {"value": args.gop * k_p / t_p, "unit": "frames/s", "ms_per_step": t_p / k_p * 1e3, "steps": k_p,
                       "dtype": {"bf16x3": "bf16 x3 split operands, f32 accumulate", "bf16x2": "bf16 x2 split, f32 accumulate",
                                 "bf16": "bf16, f32 accumulate", "f32-chain": "f32"}.get(prec, prec),
                       "scope": ("f32 everywhere; the entropy-parameter networks (context fusion, LL network, conv-LSTM) sum every "
                                 "convolution as one chain from the bias instead of ATen's per-block order, torch.sigmoid without "
                                 "the scalar tails: coefficients and motion as the reference's, CDF rows not always")
                                if prec == "f32-chain" else
                                "3x3 convolutions with 64 / 112 couts on planes >= 30 000 px, stride 1 and the stride-2 quarter-resolution context convolutions (conv_split.hip); all else f32 as in f32-chain",
                       "schedule": sched_text[args.schedule],
                       "stage_batched": {"value": args.gop * k_p / t_pb, "ms_per_step": t_pb / k_p * 1e3,
                                         "schedule": sched_text["stages"],
                                         "bits_identical_to_this_profile_pair_by_pair": last.pop("enc_b")["bits"] == e_p["bits"]},
                       "bpp": sum(e_p["bits"]) / (args.gop * W * H), "psnr_yuv": sum(p["yuv"] for p in ps_p) / len(ps_p),
                       "rel_bits_vs_exact_profile": (sum(e_p["bits"]) - sum(enc["bits"])) / sum(enc["bits"]),
                       "max_abs_dpsnr_vs_exact_profile_db": max(abs(p["yuv"] - q["yuv"]) for p, q in zip(ps_p, ps))}
                if ref_bits is not None:
                    db = np.array(e_p["bits"]) - ref_bits
                    blk["vs_reference_cpu"] = {"frames_with_identical_bits": int((db == 0).sum()), "frames": int(db.size),
                                               "max_abs_bit_delta_per_frame": float(np.abs(db).max()),
                                               "rel_total_bits": float(db.sum() / ref_bits.sum()),
                                               "max_abs_dpsnr_db": float(np.abs(np.array([p["yuv"] for p in ps_p]) - ref_psnr).max())}
                out["aux_profiles"][prec] = blk
            for prec in args.aux_precisions.split(","):
                optional("aux_profiles." + prec, lambda prec=prec: profile(prec))
            net.precision = "f32"
        if aux:     # last: it captures its launches into a graph of its own, which must not sit between the other legs
            def hbm_kernels():
                # the bandwidth-bound kernels of the path (warp, lifting add, depthwise, few-channel convs, resampling) on
                # their 1080p shapes: algorithmic bytes / HIP-event time against the 8 TB/s HBM3E peak (tools/bench_hbm.py)
                import contextlib
                import io
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import bench_hbm
                with contextlib.redirect_stdout(io.StringIO()):
                    rows = bench_hbm.main()
                out["hbm_kernels"] = {"peak_GBps": bench_hbm.PEAK, "rows": [
                    {"kernel": n, "us": round(t * 1e6, 1), "algorithmic_MB": round(b / 1e6, 1),
                     "GBps": round(b / t / 1e9), "frac_of_hbm_peak": round(b / t / 1e9 / bench_hbm.PEAK, 3)} for n, t, b in rows]}
            optional("hbm_kernels", hbm_kernels)
        if skipped:
            out["aux_skipped_over_budget"] = skipped
        out["bench_wall_s"] = time.time() - t_process
        print(json.dumps(out), flush=True)
    leave_group(dist)


def leave_group(dist):
    if dist is None:
        return
    import threading
    leave = threading.Timer(60.0, lambda: os._exit(3))      # the line is out; a barrier that never returns is a failure
    leave.daemon = True
    leave.start()
    try:
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001 - a rank that left through its watchdog
        pass


if __name__ == "__main__":
    main()
