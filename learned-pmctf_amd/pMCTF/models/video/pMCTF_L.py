"""pMCTF — variable-rate learned wavelet video coder (MCTF), MI355X-native encode path.

Drop-in for pMCTF.models.video.pMCTF_L.pMCTF of the reference (pMCTF/models/video/pMCTF_L.py): same
constructor, same parameter tree (load_state_dict(strict=True) of a reference checkpoint), same
`update`, `encode_one_stage`, `inverse_MCTF`, `get_qp_num`, `num_me_stages`, so that
test_pMCTF_flex.py runs unchanged.  All tensor arithmetic of the encode path runs in hand-written
gfx950 kernels (pMCTF.hip.engine.HipEngine -> libpmctf_hip.so); the range coder is libpmctf_rans.so
on host threads.  There is no CPU fallback: without a GPU and the built libraries the calls raise.

Implemented: the write-stream encode branch (pMCTF_L.py:553-637) with skip_decoding True or False (real decoder:
decompress_mv, decompress_one_stage), inverse_MCTF, the estimate-mode forward (forward / forward_one_stage at
inference), the estimate-only branch of encode_one_stage (output_path=None: forward_one_stage for luma and chroma; the
reference's own version raises KeyError, SURVEY F3 — here it returns what it was meant to).  Not implemented (raise
NotImplementedError): training-mode forward.  me_downsample in {1, 2, 4, 8} is supported everywhere (motion
estimated and coded at reduced resolution).
"""
import contextlib
import os
import os.path as osp
import threading
import time

import torch
from torch import nn

from pMCTF.entropy_models.entropy_models import BitEstimator
from pMCTF.entropy_models.gaussian_model import CompressionModel
from pMCTF.hip.deferred import Deferred, DeferredTensor, is_pending, unwrap
from pMCTF.hip.engine import HipEngine
from pMCTF.layers.modules import (DepthConvBlock, ME_Spynet, MvDec, MvEnc, TemporalLifting, get_hyper_dec_model,
                                  get_hyper_enc_model)
from pMCTF.models.pWave import pWave
from pMCTF.utils.stream_helper import decode_p, image_header, mv_header


def _gated(fn):
    """hold the engine's capture gate (shared) for the duration of a model entry point; re-entrant per thread"""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        tls = self._tls
        if getattr(tls, "gated", False):
            return fn(self, *a, **k)
        try:
            eng = self.engine()
        except RuntimeError:                # no GPU / update() not called: the entry point raises its own error
            return fn(self, *a, **k)
        with eng.gate.shared():
            # Launch plans are for ONE host thread driving the engine (the reference harness).  Once a second thread shows
            # up (bench.py --inflight), recording stops for good: a capture cannot coexist with another thread's device
            # synchronisations, pinned allocations or event queries, and that thread waited at the gate until the capture
            # in progress, if any, was over.
            eng.host_threads.add(threading.get_ident())
            if len(eng.host_threads) > 1:
                eng.use_graphs = False
            tls.gated = True
            try:
                return fn(self, *a, **k)
            finally:
                tls.gated = False
    return wrapper


class MVCoderQuad(nn.Module):
    """four-part MV latent coder (pMCTF/layers/video/four_part_prior.py) — parameter-free; the arithmetic is the
    pmctf_mv_fourpart_step_f32 kernel."""

    def __init__(self, enc_dec_quant=False):
        super().__init__()
        self.enc_dec_quant = enc_dec_quant


class pMCTF(nn.Module):
    def __init__(self, bitdepth=8, decomp_levels=4, lossy=True, two_stage_me=True, num_me_stages=2, quant_stage=True,
                 **kwargs):
        super().__init__()
        self.bitdepth = bitdepth
        self.dynamic_range = 2 ** bitdepth - 1
        self.lossy = lossy
        self.lp_coder = pWave(bitdepth, decomp_levels, lossy)
        self.hp_coder = pWave(bitdepth, decomp_levels, lossy)
        self.mse = nn.MSELoss(reduction="mean")
        channel_mv, channel_N, channel_M = 64, 64, 32
        self.channel_mv, self.channel_N, self.channel_M = channel_mv, channel_N, channel_M
        self.optic_flow = ME_Spynet(L=6)
        S = range(num_me_stages)
        self.mv_encoder = nn.ModuleList([MvEnc(2, channel_mv) for _ in S])
        self.mv_decoder = nn.ModuleList([MvDec(2, channel_mv) for _ in S])
        self.mv_hyper_prior_encoder = nn.ModuleList([get_hyper_enc_model(channel_N, channel_mv) for _ in S])
        self.mv_hyper_prior_decoder = nn.ModuleList([get_hyper_dec_model(channel_N, channel_mv) for _ in S])
        self.mv_y_prior_fusion_adaptor_0 = nn.ModuleList([DepthConvBlock(channel_mv, channel_mv * 2) for _ in S])
        self.mv_y_prior_fusion_adaptor_1 = nn.ModuleList([DepthConvBlock(channel_mv * 2, channel_mv * 2) for _ in S])
        self.mv_y_prior_fusion = nn.ModuleList([nn.Sequential(DepthConvBlock(channel_mv * 2, channel_mv * 3),
                                                              DepthConvBlock(channel_mv * 3, channel_mv * 3))
                                                for _ in S])
        self.mv_y_spatial_prior = nn.ModuleList([nn.Sequential(DepthConvBlock(channel_mv * 3, channel_mv * 3),
                                                               DepthConvBlock(channel_mv * 3, channel_mv * 3),
                                                               DepthConvBlock(channel_mv * 3, channel_mv * 2))
                                                 for _ in S])
        for k in (1, 2, 3):
            setattr(self, f"mv_y_spatial_prior_adaptor_{k}",
                    nn.ModuleList([nn.Conv2d(channel_mv * 4, channel_mv * 3, 1) for _ in S]))
        self.mv_y_q_scale_enc = nn.ParameterList([nn.Parameter(torch.ones((2, 1, 1, 1))) for _ in S])
        self.mv_y_q_scale_dec = nn.ParameterList([nn.Parameter(torch.ones((2, 1, 1, 1))) for _ in S])
        self.mv_bit_est = nn.ModuleList([BitEstimator(channel_mv) for _ in S])
        self.em = CompressionModel(y_distribution="laplace")
        self.mv_coder = MVCoderQuad(enc_dec_quant=True)
        self.temporal_filtering = nn.ModuleList([TemporalLifting() for _ in S])
        self.quant_stage = quant_stage
        if self.quant_stage:
            self.hp_q_scale = nn.ParameterList([nn.Parameter(torch.ones((2, 1, 1, 1))) for _ in S])
        self.two_stage_me = two_stage_me
        self.num_me_stages = num_me_stages
        self._engine = None
        # Opt-in (PMCTF_LAZY=1 / lazy_stages=True): encode_one_stage hands back DEFERRED results, the pairs a caller
        # passes one by one are collected per temporal stage and coded as one batch when a value is first needed
        # (pMCTF.hip.deferred).  Off by default: the reference harness formats a bit count after every call
        # (test_pMCTF_flex.py:240,248), which forces every pair at once, and its log step needs plain numbers
        # (video_eval_utils.py:86-133) — the default returns finished tensors and Python floats, call by call.
        # arithmetic profile of the engine: "f32" (PM-F32, the parity path), "f32-chain" (faster, approximate entropy
        # parameters) or the auxiliary reduced-precision profiles
        # "bf16x3" / "bf16x2" / "bf16" (HipEngine docstring); set before the first encode, or call update(force=True)
        self.precision = os.environ.get("PMCTF_PRECISION", "f32")
        self.lazy_stages = os.environ.get("PMCTF_LAZY", "0") == "1"
        self.lazy_max_pairs = int(os.environ.get("PMCTF_LAZY_MAX_PAIRS", "32"))
        self._tls = threading.local()
        self._atexit = False

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def get_qp_num():
        return 21

    def update(self, force=False):
        """Build the CDF tables and the range coder (pMCTF_L.py:441-446), then pack weights for the GPU."""
        self.em.update(force)
        for i in range(self.num_me_stages):
            self.mv_bit_est[i].update(force, entropy_coder=self.em.entropy_coder)
        self.lp_coder.update(force)
        self.hp_coder.update(force)
        if force:
            self._drop_engine()

    def load_state_dict(self, *args, **kwargs):
        self._drop_engine()
        return super().load_state_dict(*args, **kwargs)

    def _drop_engine(self):
        if self._engine is not None:
            self._engine.release()
        self._engine = None

    def __del__(self):
        # the engine's launch plans hold device memory pools: give them back when the model goes, not when the cyclic
        # collector gets round to the engine (which may be in the middle of another model's stream capture)
        try:
            if getattr(self, "_engine", None) is not None:
                self._drop_engine()
        except Exception:  # noqa: BLE001 - interpreter shutdown, device already gone
            pass

    def engine(self):
        if self._engine is not None and self._engine.precision != self.precision:
            self._drop_engine()
        if self._engine is None:
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise RuntimeError("pMCTF (MI355X build) encodes on the GPU only: move the model to 'cuda' "
                                   "(test_pMCTF_flex.py --cuda 1); there is no CPU path")
            ge = self.em.gaussian_encoder
            if ge.get_cdf_info()[0] is None:
                raise RuntimeError("call update(force=True) before encoding")
            g = {"cdf_info": ge.get_cdf_info(), "log_scale_min": ge.log_scale_min, "log_scale_step": ge.log_scale_step}
            z = [self.mv_bit_est[i].get_cdf_info() for i in range(self.num_me_stages)]
            self._engine = HipEngine(self.state_dict(), self.num_me_stages, dev, g, z, precision=self.precision)
        return self._engine

    # ------------------------------------------------------------------------------------------
    # deferred pairs (one queue per calling thread)
    def _queue(self):
        q = getattr(self._tls, "q", None)
        if q is None:
            q = self._tls.q = {"key": None, "pairs": [], "dpb0": None}
        return q

    def _pending_files(self):
        p = getattr(self._tls, "files", None)
        if p is None:
            p = self._tls.files = []
        return p

    def flush(self):
        """Code every pair collected so far and wait for the range-coder threads: the bitstream files of every pair handed
        over so far exist from here on.  (Using a deferred bit count waits for that pair's files; using a deferred
        tensor only enqueues the GPU work.)"""
        self._run_pending()
        files, self._tls.files = self._pending_files(), []
        first = None
        for f in files:
            try:
                f.result()
            except BaseException as e:  # noqa: BLE001 - wait for every writer, then report the first failure
                first = first or e
        if first is not None:
            raise first

    def _run_pending(self, q=None):
        """Enqueue the GPU work of every pair collected so far (one encode_stage_pairs call); does not wait for the
        range coder."""
        q = self._queue() if q is None else q
        recs, q["pairs"] = q["pairs"], []
        if not recs:
            return
        key, dpb0, q["key"], q["dpb0"] = q["key"], q["dpb0"], None, None
        code_lt, stage_idx, q_index, psize, pic_width, pic_height, me_downsample = key[:7]
        try:
            results, _ = self.encode_stage_pairs([r["pair"] for r in recs], code_lt, dpb0, [r["path"] for r in recs],
                                                 pic_width, pic_height, psize=psize, stage_idx=stage_idx, q_index=q_index,
                                                 chain_reset=[i for i, r in enumerate(recs) if r["reset"] and i > 0],
                                                 me_downsample=me_downsample, wait_files=False)
        except BaseException as e:
            for r in recs:
                r["error"] = e
            raise
        for r, res in zip(recs, results):
            r["result"] = res

    def _defer(self, ref_frame, cur_frame, code_lt, dpb, output_path, pic_width, pic_height, psize, stage_idx, q_index,
               me_downsample=1):
        q = self._queue()
        if not self._atexit:
            # deferred pairs still queued when the interpreter exits are coded then (their files must exist)
            import atexit
            import weakref
            ref = weakref.ref(self)
            atexit.register(lambda: ref() is not None and ref().flush())
            self._atexit = True
        # inputs produced by pairs that are still pending (a later temporal stage): they are needed now
        if any(is_pending(t) for t in (*ref_frame, *cur_frame)):
            self._run_pending()
        ref_frame, cur_frame = unwrap(list(ref_frame)), unwrap(list(cur_frame))
        key = (code_lt, stage_idx, q_index, psize, pic_width, pic_height, me_downsample, tuple(ref_frame[0].shape),
               tuple(ref_frame[1].shape), ref_frame[0].device)
        mvf, rmy = dpb["mv_feature"], dpb["ref_mv_y"]
        last = q["pairs"][-1] if q["pairs"] else None
        chained = last is not None and mvf is last["out"]["dpb"]["mv_feature"] and rmy is last["out"]["dpb"]["ref_mv_y"]
        fresh = mvf is None and rmy is None
        if q["pairs"] and (key != q["key"] or not (chained or fresh) or len(q["pairs"]) >= self.lazy_max_pairs):
            self._run_pending()
            chained = False
        if not q["pairs"]:
            q["key"] = key
            q["dpb0"] = {"mv_feature": unwrap(mvf), "ref_mv_y": unwrap(rmy)}
        rec = {"pair": (ref_frame, cur_frame), "path": output_path, "reset": fresh and not chained, "result": None,
               "error": None}

        def get(k, sub=None):
            def thunk():
                if rec["result"] is None:
                    if rec["error"] is not None:
                        raise RuntimeError("the deferred encode of this pair failed") from rec["error"]
                    self._run_pending(q)
                v = rec["result"][k]
                return v[sub] if sub is not None else v
            return thunk
        ready = lambda: rec["result"] is not None
        out = {k: DeferredTensor(get(k), ready) for k in ("L_t", "H_t", "L_tc", "H_tc", "mv_hat")}
        for k in ("bit_H", "bit_Hc", "bit_ME", "encoding_time"):
            out[k] = Deferred(get(k), ready)
        out["bit_L"] = Deferred(get("bit_L"), ready) if code_lt else None
        out["bit_Lc"] = Deferred(get("bit_Lc"), ready) if code_lt else None
        out["dpb"] = {"mv_feature": DeferredTensor(get("dpb", "mv_feature"), ready),
                      "ref_mv_y": DeferredTensor(get("dpb", "ref_mv_y"), ready)}
        out["decoding_time"] = 0
        if self.engine().keep_streams:
            out["files"], out["traces"] = Deferred(get("files"), ready), Deferred(get("traces"), ready)
        rec["out"] = out
        q["pairs"].append(rec)
        return out

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    @_gated
    def inverse_MCTF(self, L_t, H_t, mv_hat, downscale=False, stage_idx=0):
        """pMCTF_L.py:314-330"""
        L_t, H_t, mv_hat = unwrap((L_t, H_t, mv_hat))
        c = lambda t: t.contiguous()
        return self.engine().inverse_MCTF(c(L_t), c(H_t), c(mv_hat), downscale=downscale, stage_idx=stage_idx)

    @torch.no_grad()
    @_gated
    def inverse_MCTF_ref(self, L_t, H_t, mv_hat, downscale=False, stage_idx=0):
        """inverse_MCTF(...)[0] without the predict half: the same tensor, bit for bit"""
        L_t, H_t, mv_hat = unwrap((L_t, H_t, mv_hat))
        c = lambda t: t.contiguous()
        return self.engine().inverse_MCTF_ref(c(L_t), c(H_t), c(mv_hat), downscale=downscale, stage_idx=stage_idx)

    @torch.no_grad()
    @_gated
    def forward_MCTF(self, ref_frame, cur_frame, mv_hat, stage_idx=0):
        """pMCTF_L.py:297-312"""
        ref_frame, cur_frame, mv_hat = unwrap((ref_frame, cur_frame, mv_hat))
        c = lambda t: t.contiguous()
        return self.engine().forward_MCTF(c(ref_frame), c(cur_frame), c(mv_hat), stage_idx)

    @staticmethod
    def _check_ds(me_downsample):
        if me_downsample not in (1, 2, 4, 8):
            raise ValueError("me_downsample must be 1, 2, 4 or 8")

    @torch.no_grad()
    @_gated
    def decompress_mv(self, string, dtype, height, width, dpb, stage_idx=0, q_index=0, me_downsample=1):
        """pMCTF_L.py:497-523 — returns mv_hat (1,2,H,W) and the MV decoder contexts (logical NCHW views)"""
        self._check_ds(me_downsample)
        dpb = unwrap(dpb)
        d = self.engine().decompress_mv(string, height, width, dpb, stage_idx=stage_idx, q_index=q_index,
                                        me_downsample=me_downsample)
        return {"mv_hat": d["mv_hat"], "mv_feature": d["mv_feature"].permute(0, 3, 1, 2),
                "mv_y_hat": d["mv_y_hat"].permute(0, 3, 1, 2)}

    @torch.no_grad()
    @_gated
    def decompress_one_stage(self, file_name, code_lt, ischroma, psize=128, q_index=0, stage_idx=0, spatial_level=0):
        """pMCTF_L.py:422-439; spatial_level=k: the planes of spatial level k (HipEngine.pwave_decompress_end)"""
        return self._decompress_files([(file_name, ischroma)], code_lt, psize, q_index, stage_idx, spatial_level)[0]

    def _decompress_files(self, files, code_lt, psize, q_index, stage_idx, spatial_level=0):
        """H (and L) files of the given (file_name, ischroma) entries; their sequential LL parts decode concurrently"""
        return self._decompress_files_end(self._decompress_files_begin(files, code_lt, psize, q_index, stage_idx,
                                                                       spatial_level))

    def _decompress_files_begin(self, files, code_lt, psize, q_index, stage_idx, spatial_level=0):
        """read the files and start their sequential LL decodes on side streams (finish with _decompress_files_end)"""
        from pMCTF.hip.engine import get_curr_q
        self.flush()            # the files of deferred pairs must exist before they are read
        eng = self.engine()
        qp_scale = get_curr_q(eng.sd[f"hp_q_scale.{stage_idx}"], q_index) if self.quant_stage else None
        jobs = []
        for file_name, ischroma in files:
            pad = psize // 2 if ischroma else psize
            with open(file_name, "rb") as f:
                jobs.append(("hp_coder", f.read(), pad, q_index, qp_scale))
            if code_lt:
                file_name_l = file_name.replace(osp.basename(file_name), "0_C_main.bin" if ischroma else "0_main.bin")
                with open(file_name_l, "rb") as f:
                    jobs.append(("lp_coder", f.read(), pad, q_index, None))
        return files, code_lt, eng.pwave_decompress_many_begin(jobs, spatial_level)

    def _decompress_files_end(self, begun):
        files, code_lt, jobs = begun
        planes = self.engine().pwave_decompress_many_end(jobs)
        out, i = [], 0
        for _ in files:
            H_t = planes[i]; i += 1
            L_t = None
            if code_lt:
                L_t = {"x_hat": planes[i]}; i += 1
            out.append({"L_t": L_t, "H_t": {"x_hat": H_t}})
        return out

    @torch.no_grad()
    @_gated
    def decompress_gop_files(self, files, psize=128, q_index=0, ll_order="position", spatial_level=0):
        """Picture files of any number of pairs and stages in one call.  files: [(data, ischroma, low, stage_idx)] — the
        bytes of one file, whether it holds the two chroma planes, whether it is an L file (lp_coder) or an H file
        (hp_coder, de-quantised with stage_idx's scale).  Returns the x_hat planes in the order of `files`.
        ll_order: see HipEngine.pwave_decompress_batch_begin.  spatial_level=k: every plane at spatial level k,
        1/2^k of its size (HipEngine.pwave_decompress_end)."""
        return self._decompress_gop_files_end(self._decompress_gop_files_begin(files, psize, q_index, ll_order,
                                                                               spatial_level=spatial_level))

    @torch.no_grad()
    @_gated
    def _decompress_gop_files_begin(self, files, psize, q_index, ll_order, names=None, spatial_level=0):
        """start the sequential LL decodes of all files (batched per geometry); finish with _decompress_gop_files_end.
        The first entry of what it returns is the list of the engine's records, one per file in order, which hold
        "symbols_decoded" and "payload_bytes_used" once the files are finished."""
        from pMCTF.hip.engine import get_curr_q
        self.flush()
        eng = self.engine()
        jobs = []
        for data, ischroma, low, stage_idx in files:
            pad = psize // 2 if ischroma else psize
            qp_scale = None
            if not low and self.quant_stage:
                qp_scale = get_curr_q(eng.sd[f"hp_q_scale.{stage_idx}"], q_index)
            jobs.append(("lp_coder" if low else "hp_coder", data, pad, q_index, qp_scale))
        return eng.pwave_decompress_batch_begin(jobs, ll_order, spatial_level), names

    @torch.no_grad()
    @_gated
    def _decompress_gop_files_end(self, begun):
        jobs, names = begun
        return self.engine().pwave_decompress_batch_end(jobs, names)

    @torch.no_grad()
    @_gated
    def encode_stage_pairs(self, pairs, code_lt, dpb, output_paths, pic_width, pic_height, psize=128, stage_idx=0,
                           q_index=0, chain_reset=(), me_downsample=1, wait_files=True):
        """All pairs of one temporal stage in one call: pairs = [(ref_frame, cur_frame)], output_paths = ["k.bin"].
        Returns ([result dict per pair, exactly what encode_one_stage(skip_decoding=True) returns for it], dpb for a
        following call).  The motion codec runs pair after pair (its context is a chain, pMCTF_L.py:448-495); the
        temporal lifting and the spatial coders — 93 % of the work — run as ONE batch over the pairs, so every launch
        is len(pairs) times larger (the MI355X-side answer to the small, latency-bound subbands of the wavelet
        pyramid; 288 GB of HBM hold the larger activations easily).  Files, bits and tensors are identical to calling
        encode_one_stage pair by pair (tests/test_gpu_engine.py::test_batched_stage_equals_pair_by_pair).
        chain_reset: indexes of pairs at which the motion context restarts from the empty one — the first pair of every
        further closed GOP when the same stage of several GOPs is coded in one call (pmctf_gop.encode_gops_batched)."""
        eng = self.engine()
        dev = next(self.parameters()).device
        pairs, dpb = unwrap(list(pairs)), unwrap(dpb)
        c = lambda t: t.to(dev).contiguous()
        start = time.time()
        keep = eng.keep_streams
        P = len(pairs)
        jobs = [dict() for _ in range(P)]
        mvs = []
        chain_reset = set(chain_reset)
        # The motion chain of this stage (SpyNet + motion codec per pair: small, latency-bound launches, 7 % of the work)
        # needs nothing of the previous stage but its uncoded L frames, which exist long before that stage's entropy
        # networks have finished.  It therefore runs on a side stream that waits only for the event recorded behind the
        # previous stage's temporal lifting, and overlaps with the previous stage's remaining work; the lifting and the
        # spatial coders of this stage (main stream) wait for it.
        main = torch.cuda.current_stream(dev)
        lumas = [c(t) for (ry, _), (cy, _) in pairs for t in (ry, cy)]
        overlap = eng.motion_overlap
        if overlap:
            side = eng.motion_stream
            lt_event, lt_tensor = eng.lt_event, eng.lt_tensor      # one snapshot: another host thread may replace them
            if lt_event is not None and eng.lt_stream == main.cuda_stream and \
                    all(t is lt_tensor or t._base is lt_tensor for t in lumas):
                side.wait_event(lt_event)            # inputs are slices of the previous stage's batched L_t
            else:
                side.wait_stream(main)
            for t in lumas:
                t.record_stream(side)
            if dpb["mv_feature"] is not None:
                side.wait_stream(main)
        ctx = torch.cuda.stream(side) if overlap else contextlib.nullcontext()
        with ctx:
            for i in range(P):
                if i in chain_reset:
                    dpb = {"mv_feature": None, "ref_mv_y": None}
                mv = eng.compress_mv(lumas[2 * i], lumas[2 * i + 1], dpb, stage_idx=stage_idx, q_index=q_index,
                                     me_downsample=me_downsample)
                jobs[i]["mv"] = eng.coder.submit(mv["stream"], eng.tables, lambda n: mv_header(n, 0),
                                                 output_paths[i].replace(".bin", "_mv.bin"), keep)
                dpb = {"mv_feature": mv["mv_feature"].permute(0, 3, 1, 2), "ref_mv_y": mv["mv_y_hat"].permute(0, 3, 1, 2)}
                mvs.append((mv, dpb))
        if overlap:
            main.wait_stream(side)
            for mv, _ in mvs:
                for k in ("mv_hat", "mv_feature", "mv_y_hat"):
                    mv[k].record_stream(main)

        def paths_for(i, kind, chroma):
            base = osp.basename(output_paths[i])
            if kind == "H":
                return output_paths[i].replace(".bin", "_C_main.bin") if chroma else output_paths[i]
            return output_paths[i].replace(base, "0_C_main.bin" if chroma else "0_main.bin")

        def submitter(chroma):
            def submit(kind, stream, n):
                if chroma:
                    hdr = lambda m: image_header(pic_height // 2, pic_width // 2, 2, m)
                else:
                    hdr = lambda m: image_header(pic_height, pic_width, 1, m)
                groups = [(i * n, n, hdr, paths_for(i, kind, chroma)) for i in range(P)]
                for i, fut in enumerate(eng.coder.submit_planes(stream, P * n, groups, eng.tables, keep)):
                    jobs[i][kind + ("c" if chroma else "")] = fut
            return submit

        mv_hats = [m["mv_hat"] for m, _ in mvs]
        def code(chroma_flag):
            k = 1 if chroma_flag else 0
            r = eng.compress_stage_batched([c(rf[k]) for rf, _ in pairs], [c(cu[k]) for _, cu in pairs], code_lt,
                                           mv_hats, chroma_flag, stage_idx, q_index, on_stream=submitter(chroma_flag))
            return r

        if eng.multi_stream and P <= eng.multi_stream_max_pairs:
            # the late stages have few pairs: luma and chroma (independent once the motion is known) share the GPU on
            # two streams so that the small launches of one fill the gaps of the other
            main = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(main)
            outs = []
            for side, flag in zip(eng.side_streams, (False, True)):
                side.wait_event(ready)
                with torch.cuda.stream(side):
                    r = code(flag)
                    r["finish"]()
                    outs.append(r)
            for side in eng.side_streams[:2]:
                main.wait_stream(side)
            luma, chroma = outs
            for r in outs:
                for k in ("L_t", "H_t", "H_t_hat", "L_t_hat"):
                    if r[k] is not None:
                        r[k].record_stream(main)
        else:
            luma = code(False)
            chroma = code(True)
            luma["finish"]()
            chroma["finish"]()
        results = []
        pending = self._pending_files()
        for f in [f for f in pending if f.done()]:
            f.result()                      # a writer thread's error (e.g. an unwritable folder) surfaces here, not never
        pending[:] = [f for f in pending if not f.done()]
        for i in range(P):
            # Bit counts are the sizes of the files the range-coder threads are still writing.  wait_files=True (a direct
            # call): wait for them here.  From the deferred drop-in path they stay deferred too, so that the host goes on
            # to enqueue the next stage while this one is still being coded (what lets its motion chain overlap).
            if wait_files:
                done = {k: j.result() for k, j in jobs[i].items()}
                bits = {k: v[0] * 8.0 for k, v in done.items()}
            else:
                pending.extend(jobs[i].values())
                done = {k: (Deferred(lambda j=j: j.result()[0]), Deferred(lambda j=j: j.result()[1]),
                            Deferred(lambda j=j: j.result()[2])) for k, j in jobs[i].items()}
                bits = {k: Deferred(lambda j=j: j.result()[0] * 8.0) for k, j in jobs[i].items()}
            mv, dpb_i = mvs[i]
            ys, cs = slice(i, i + 1), slice(2 * i, 2 * i + 2)
            r = {"L_t": (luma["L_t_hat"] if code_lt else luma["L_t"])[ys], "H_t": luma["H_t_hat"][ys],
                 "L_tc": (chroma["L_t_hat"] if code_lt else chroma["L_t"])[cs], "H_tc": chroma["H_t_hat"][cs],
                 "bit_H": bits["H"] + bits["Hc"], "bit_L": bits["L"] + bits["Lc"] if code_lt else None,
                 "bit_Hc": bits["Hc"], "bit_Lc": bits["Lc"] if code_lt else None, "bit_ME": bits["mv"],
                 "mv_hat": mv["mv_hat"], "dpb": dpb_i, "decoding_time": 0, "encoding_time": None}
            if keep:
                r["files"] = {k: v[1] for k, v in done.items()}
                r["traces"] = {k: v[2] for k, v in done.items()}
            results.append(r)
        eng.stats["pair_s"] += time.time() - start
        eng.stats["pairs"] += P
        for r in results:
            r["encoding_time"] = (time.time() - start) / P
        return results, dpb

    @staticmethod
    def dpb_shapes(height, width, me_downsample=1):
        """logical NCHW shapes of the motion codec's context (mv_feature, ref_mv_y) for planes of height x width"""
        h, w = height // me_downsample, width // me_downsample
        return [(1, 64, h // 4, w // 4), (1, 64, h // 16, w // 16)]

    @torch.no_grad()
    @_gated
    def advance_dpb(self, ref_frame, cur_frame, dpb, stage_idx=0, q_index=0, me_downsample=1):
        """The motion part of encode_one_stage only (pMCTF_L.py:448-495): returns the `dpb` the NEXT pair of the stage
        needs.  Used by pair-level sharding (pmctf_dist.encode_gop_pair_sharded): the context chain of the motion codec
        is the only dependency between the pairs of a stage, and a rank re-computes it rather than waiting for it."""
        self._check_ds(me_downsample)
        ref_frame, cur_frame, dpb = unwrap((list(ref_frame), list(cur_frame), dpb))
        eng = self.engine()
        dev = next(self.parameters()).device
        c = lambda t: t.to(dev).contiguous()
        mv = eng.compress_mv(c(ref_frame[0]), c(cur_frame[0]), dpb, stage_idx=stage_idx, q_index=q_index,
                             me_downsample=me_downsample)
        return {"mv_feature": mv["mv_feature"].permute(0, 3, 1, 2), "ref_mv_y": mv["mv_y_hat"].permute(0, 3, 1, 2)}

    # ---- a frame pair in PARTS (pmctf_dist: ranks that a temporal stage leaves idle share the pairs it has) ------------
    # encode_one_stage's write branch = motion (SpyNet + motion codec -> mv_hat, {k}_mv.bin), then four spatial coder calls
    # that are independent given mv_hat (pMCTF_L.py:398-420,570-592): H and L of luma, H and L of chroma.  The two methods
    # below run those pieces on their own, through the same engine code (stream launches), so that the union of the
    # parts of a pair — whichever ranks run them — is encode_one_stage's result: same files, bits and tensors
    # (tests/test_gpu_engine.py::test_pair_parts_equal_encode_one_stage).
    @torch.no_grad()
    @_gated
    def encode_pair_motion(self, ref_frame, cur_frame, dpb, output_path, stage_idx=0, q_index=0, me_downsample=1,
                           on_dpb=None):
        """Motion of one pair: writes {k}_mv.bin.  dpb / on_dpb as in encode_one_stage.  -> {mv_hat, dpb, bit_ME}"""
        self._check_ds(me_downsample)
        self.flush()
        ref_frame, cur_frame = unwrap((list(ref_frame), list(cur_frame)))
        eng = self.engine()
        dev = ref_frame[0].device
        c = lambda t: t.to(dev).contiguous()
        mv = eng.compress_mv(c(ref_frame[0]), c(cur_frame[0]), dpb if callable(dpb) else unwrap(dpb), stage_idx=stage_idx,
                             q_index=q_index, me_downsample=me_downsample)
        job = eng.coder.submit(mv["stream"], eng.tables, lambda n: mv_header(n, 0), output_path.replace(".bin", "_mv.bin"),
                               eng.keep_streams)
        new = {"mv_feature": mv["mv_feature"].permute(0, 3, 1, 2), "ref_mv_y": mv["mv_y_hat"].permute(0, 3, 1, 2)}
        if on_dpb is not None:
            on_dpb(new)
        return {"mv_hat": mv["mv_hat"], "dpb": new, "bit_ME": job.result()[0] * 8.0}

    @torch.no_grad()
    @_gated
    def encode_pair_part(self, ref_planes, cur_planes, mv_hat, chroma, kinds, code_lt, output_path, pic_width, pic_height,
                         stage_idx=0, q_index=0):
        """The spatial coders `kinds` (a subset of ("H", "L"); "L" only where the stage codes L) of the luma (chroma=False:
        planes (1,1,H,W)) or chroma (True: (2,1,H/2,W/2)) planes of one pair, given the pair's decoded motion field.
        Writes the files encode_one_stage would ({k}.bin / {k}_C_main.bin, 0_main.bin / 0_C_main.bin).
        -> {"H": reconstructed H planes or None, "L": the L planes this part is responsible for — coded and reconstructed
        if "L" in kinds, the temporal low-pass itself where the stage does not code L, else None, "bits": {kind: bits}}"""
        self.flush()
        ref_planes, cur_planes, mv_hat = unwrap((ref_planes, cur_planes, mv_hat))
        eng = self.engine()
        dev = ref_planes.device
        c = lambda t: t.to(dev).contiguous()
        base = osp.basename(output_path)
        if chroma:
            paths = {"H": output_path.replace(".bin", "_C_main.bin"), "L": output_path.replace(base, "0_C_main.bin")}
            header = lambda n: image_header(pic_height // 2, pic_width // 2, 2, n)
        else:
            paths = {"H": output_path, "L": output_path.replace(base, "0_main.bin")}
            header = lambda n: image_header(pic_height, pic_width, 1, n)
        assert set(kinds) <= {"H", "L"} and ("L" not in kinds or code_lt)
        jobs = {}

        def submit(kind, stream):
            jobs[kind] = eng.coder.submit(stream, eng.tables, header, paths[kind], eng.keep_streams)
        out = eng.compress_one_stage(c(ref_planes), c(cur_planes), bool(code_lt) and "L" in kinds, c(mv_hat), bool(chroma),
                                     stage_idx, q_index, False, on_stream=submit, defer=True, code_h="H" in kinds)
        out["finish"]()
        low = out["L_t_hat"] if "L" in kinds else (out["L_t"] if not code_lt else None)
        return {"H": out["H_t_hat"], "L": low, "bits": {k: j.result()[0] * 8.0 for k, j in jobs.items()}}

    @torch.no_grad()
    @_gated
    def encode_lone_picture(self, frame, output_folder, pic_width, pic_height, psize=128, skip_decoding=True, q_index=0):
        """A picture with no partner (a GOP of one, pmctf_seq): frame = [Y (1,1,Hp,Wp), UV (2,1,Hp/2,Wp/2)] padded planes,
        coded by the L coder alone exactly as the L picture of a pair is (no motion, no temporal lifting, no H file).
        Writes output_folder/0_main.bin and 0_C_main.bin with the framing of every other L picture; with
        skip_decoding=False the LL symbols are in the sequential decoder's order and the returned planes are decoded from
        the files, as in encode_one_stage.
        -> {"L_t", "L_tc": reconstructed planes, "bit_L": 8 x both files' bytes, "bit_Lc": the chroma file's share,
            "encoding_time", "decoding_time"}"""
        self.flush()
        y, c = unwrap(list(frame))
        eng = self.engine()
        start = time.time()
        paths = {False: osp.join(output_folder, "0_main.bin"), True: osp.join(output_folder, "0_C_main.bin")}
        headers = {False: lambda n: image_header(pic_height, pic_width, 1, n),
                   True: lambda n: image_header(pic_height // 2, pic_width // 2, 2, n)}
        jobs, synth = {}, {}
        for chroma, planes in ((False, y), (True, c)):
            synth[chroma], stream = eng.pwave_compress("lp_coder", planes.contiguous().float(), q_index, None,
                                                       not skip_decoding, defer=True)
            jobs[chroma] = eng.coder.submit(stream, eng.tables, headers[chroma], paths[chroma], eng.keep_streams)
        rec = {chroma: fn() for chroma, fn in synth.items()}
        bits = {chroma: j.result()[0] * 8.0 for chroma, j in jobs.items()}
        encoding_time = time.time() - start
        decoding_time = 0
        if not skip_decoding:
            t0 = time.time()
            files = []
            for chroma in (False, True):
                with open(paths[chroma], "rb") as f:
                    files.append((f.read(), chroma, True, 0))
            rec[False], rec[True] = self.decompress_gop_files(files, psize=psize, q_index=q_index, ll_order="position")
            torch.cuda.synchronize()
            decoding_time = time.time() - t0
        return {"L_t": rec[False], "L_tc": rec[True], "bit_L": bits[False] + bits[True], "bit_Lc": bits[True],
                "encoding_time": encoding_time, "decoding_time": decoding_time}

    @torch.no_grad()
    @_gated
    def forward_one_stage(self, ref_frame, cur_frame, q_index, code_lt, dpb, mv_hat=None, stage_idx=0, me_downsample=1):
        """Estimate-mode stage (pMCTF_L.py:332-379): the same networks as encode_one_stage with Laplace / factorized
        bit estimates instead of range coding.  ref_frame / cur_frame are (N,1,H,W) planes (Y, or UV with the luma
        motion passed as mv_hat).  Scalars come back as 0-dim float32 CPU tensors (one device read per call)."""
        self._check_ds(me_downsample)
        if self.training:
            raise NotImplementedError("training forward (noise quantisation, gradients) is not part of this build")
        ref_frame, cur_frame, dpb, mv_hat = unwrap((ref_frame, cur_frame, dpb, mv_hat))
        eng = self.engine()
        dev = next(self.parameters()).device
        ref, cur = ref_frame.to(dev).contiguous(), cur_frame.to(dev).contiguous()
        r = eng.forward_one_stage(ref, cur, q_index, code_lt, dpb, None if mv_hat is None else mv_hat.contiguous(),
                                  stage_idx, me_downsample)
        acc = r["acc"]
        keys = sorted(acc)
        vals = torch.cat([acc[k].reshape(-1).sum().reshape(1) for k in keys]).cpu().tolist()     # the one sync
        v = dict(zip(keys, vals))
        N, _, H, W = ref.shape
        pix = H * W
        t = lambda x: None if x is None else torch.tensor(x, dtype=torch.float32)
        has_mv = "bits_mv_y" in v
        bpp_y = v["bits_mv_y"] / pix if has_mv else None
        bpp_z = v["bits_mv_z"] / pix if has_mv else None
        bpp_H = v["bits_H"] / (pix * N)
        bpp = bpp_H + bpp_z + bpp_y if has_mv else bpp_H
        nchw = lambda x: None if x is None else x.permute(0, 3, 1, 2)
        ret = {"bpp_mv_y": t(bpp_y), "bpp_mv_z": t(bpp_z), "bpp_me": t(bpp_z + bpp_y) if has_mv else None,
               "me_mse": t(v["sq_me"] / (pix * N)), "bpp": t(bpp), "bpp_H": t(bpp_H), "bit_H": t(v["bits_H"] / N),
               "bit_ME": t((bpp_y + bpp_z) * pix) if has_mv else None, "mse_H": t(v["sq_H"] / (pix * N)),
               "mv_hat": r["mv_hat"],
               "dpb": {"mv_feature": nchw(r["ref_mv"]["mv_feature"]), "ref_mv_y": nchw(r["ref_mv"]["mv_y_hat"])},
               "H_t": r["H_t"], "L_t": r["L_t"]}
        if code_lt:
            ret.update({"bpp_L": t(v["bits_L"] / (pix * N)), "bit_L": t(v["bits_L"] / N),
                        "mse_L": t(v["sq_L"] / (pix * N)), "me_mse_inv": t(v["sq_me_inv"] / (pix * N))})
        ret["bit"] = t(bpp * pix)
        return ret

    def forward(self, ref_frame, cur_frame, q_index, code_lt, dpb, stage_idx=0):
        """pMCTF_L.py:294-295"""
        return self.forward_one_stage(ref_frame, cur_frame, q_index, code_lt, dpb, stage_idx=stage_idx)

    @torch.no_grad()
    @_gated
    def encode_one_stage(self, ref_frame, cur_frame, code_lt, dpb, output_path=None, pic_width=None, pic_height=None,
                         psize=128, skip_decoding=False, stage_idx=0, q_index=0, me_downsample=1, on_dpb=None):
        """Write-stream branch of pMCTF_L.py:525-637 for one frame pair.
        Beyond the reference's signature (used by pmctf_dist's relay only): `dpb` may be a zero-argument callable that
        delivers the context once the motion has been estimated, and `on_dpb(dpb)` is called with the NEXT pair's
        context as soon as the motion codec has produced it, before the subbands are coded."""
        self._check_ds(me_downsample)
        if self.lazy_stages and output_path is not None and skip_decoding and on_dpb is None and not callable(dpb):
            return self._defer(ref_frame, cur_frame, code_lt, dpb, output_path, pic_width, pic_height, psize, stage_idx,
                               q_index, me_downsample)
        self.flush()
        ref_frame, cur_frame = unwrap((list(ref_frame), list(cur_frame)))
        if not callable(dpb):
            dpb = unwrap(dpb)
        if output_path is None:
            # Estimate-only branch (pMCTF_L.py:530-551): the same networks with Laplace / factorized bit estimates, no
            # range coding.  The reference builds `dpb` from result["mv_feature"] / result["ref_mv_y"], keys that
            # forward_one_stage does not return (KeyError); what it was meant to hand on is
            # forward_one_stage's own "dpb", which is what is returned here.
            if callable(dpb):
                dpb = dpb()
            ry = self.forward_one_stage(ref_frame[0], cur_frame[0], q_index, code_lt, dpb, stage_idx=stage_idx,
                                        me_downsample=me_downsample)
            rc = self.forward_one_stage(ref_frame[1], cur_frame[1], q_index, code_lt, dpb, mv_hat=ry["mv_hat"],
                                        stage_idx=stage_idx, me_downsample=me_downsample)
            if on_dpb is not None:
                on_dpb(ry["dpb"])
            return {"L_t": ry["L_t"], "H_t": ry["H_t"], "L_tc": rc["L_t"], "H_tc": rc["H_t"],
                    "bit_L": ry["bit_L"] + rc["bit_L"] if code_lt else None, "bit_H": ry["bit_H"] + rc["bit_H"],
                    "bit_Lc": rc["bit_L"] if code_lt else None, "bit_Hc": rc["bit_H"], "bit_ME": ry["bit_ME"],
                    "mv_hat": ry["mv_hat"], "dpb": ry["dpb"], "decoding_time": 0, "encoding_time": 0}
        eng = self.engine()
        ref_y, ref_chroma = ref_frame
        cur_y, cur_chroma = cur_frame
        dev = ref_y.device
        c = lambda t: t.to(dev).contiguous()
        plan_key = None
        relayed = callable(dpb) or on_dpb is not None
        if eng.use_graphs and skip_decoding and dev.type == "cuda":
            chained = callable(dpb) or dpb["mv_feature"] is not None
            plan_key = (threading.get_ident(), tuple(ref_y.shape), tuple(ref_chroma.shape), chained, bool(code_lt), stage_idx,
                        q_index, me_downsample)
            plan = eng.pair_plans.get(plan_key)
            if plan is not None:
                return self._encode_pair_planned(plan, c(ref_y), c(cur_y), c(ref_chroma), c(cur_chroma), code_lt, dpb,
                                                 output_path, pic_width, pic_height, on_dpb)
        start = time.time()
        keep = eng.keep_streams
        mv_out = output_path.replace(".bin", "_mv.bin")
        if callable(dpb):
            deliver, got = dpb, {}

            def dpb():
                got["dpb"] = deliver()
                return got["dpb"]
            mv = eng.compress_mv(c(ref_y), c(cur_y), dpb, stage_idx=stage_idx, q_index=q_index,
                                 me_downsample=me_downsample)
            dpb = got["dpb"]
        else:
            mv = eng.compress_mv(c(ref_y), c(cur_y), dpb, stage_idx=stage_idx, q_index=q_index,
                                 me_downsample=me_downsample)
        jobs = {"mv": eng.coder.submit(mv["stream"], eng.tables, lambda n: mv_header(n, 0), mv_out, keep)}
        mv_hat = mv["mv_hat"]
        if on_dpb is not None:
            on_dpb({"mv_feature": mv["mv_feature"].permute(0, 3, 1, 2), "ref_mv_y": mv["mv_y_hat"].permute(0, 3, 1, 2)})
        base = osp.basename(output_path)
        file_name_c = output_path.replace(".bin", "_C_main.bin")
        ry, cy, rc, cc = c(ref_y), c(cur_y), c(ref_chroma), c(cur_chroma)

        # Each stream goes to the range coder the moment its symbols are complete; the synthesis side of the four coders
        # (inverse DWT + post-processing, needed only for the returned reconstructions) runs after all streams have
        # been submitted, so the coder's tail overlaps with GPU work.
        def code_luma():
            paths = {"H": output_path, "L": output_path.replace(base, "0_main.bin")}

            def submit(kind, stream):
                jobs[kind] = eng.coder.submit(stream, eng.tables, lambda n: image_header(pic_height, pic_width, 1, n),
                                              paths[kind], keep)
            return eng.compress_one_stage(ry, cy, code_lt, mv_hat, False, stage_idx, q_index, not skip_decoding,
                                          on_stream=submit, defer=True)

        def code_chroma():
            paths = {"H": file_name_c, "L": output_path.replace(base, "0_C_main.bin")}

            def submit(kind, stream):
                jobs[kind + "c"] = eng.coder.submit(stream, eng.tables,
                                                    lambda n: image_header(pic_height // 2, pic_width // 2, 2, n),
                                                    paths[kind], keep)
            return eng.compress_one_stage(rc, cc, code_lt, mv_hat, True, stage_idx, q_index, not skip_decoding,
                                          on_stream=submit, defer=True)

        if eng.multi_stream:
            main = torch.cuda.current_stream()
            ready = torch.cuda.Event()
            ready.record(main)
            outs = []
            for side, fn in zip(eng.side_streams, (code_luma, code_chroma)):
                side.wait_event(ready)
                with torch.cuda.stream(side):
                    outs.append(fn()["finish"]())
            for side in eng.side_streams:
                main.wait_stream(side)
            luma, chroma = outs
            for r in outs:                 # results are consumed on the caller's stream from now on
                for k in ("L_t", "H_t", "H_t_hat", "L_t_hat"):
                    if r[k] is not None:
                        r[k].record_stream(main)
        else:
            luma = code_luma()
            chroma = code_chroma()
            luma["finish"]()
            chroma["finish"]()
        t_enq = time.time() - start
        if eng.profile_host:
            torch.cuda.synchronize()
            eng.stats["gpu_done_s"] += time.time() - start
        done = {k: j.result() for k, j in jobs.items()}
        eng.stats["enqueue_s"] += t_enq
        eng.stats["pair_s"] += time.time() - start
        eng.stats["pairs"] += 1
        encoding_time = time.time() - start
        bits = {k: v[0] * 8.0 for k, v in done.items()}
        decoding_time = 0
        mv_feature = mv["mv_feature"]
        if not skip_decoding:
            # pMCTF_L.py:594-612: hand back what the decoder reconstructs from the files just written
            t0 = time.time()
            mv_y_q_index, string = decode_p(mv_out)
            # (the reference passes the full-resolution size and no factor here, pMCTF_L.py:597-602, which cannot
            # decode a reduced-resolution motion stream; the stream is decoded at the size it was coded at)
            # the pictures' sequential LL parts start first (one CU each, side streams): the motion stream decodes under them
            begun = self._decompress_files_begin([(output_path, False), (file_name_c, True)], code_lt, psize, q_index,
                                                 stage_idx)
            decoded = self.decompress_mv(string, ref_y.dtype, ref_y.size(2) // me_downsample,
                                         ref_y.size(3) // me_downsample, dpb, stage_idx=stage_idx, q_index=q_index,
                                         me_downsample=me_downsample)
            mv_hat = decoded["mv_hat"]
            mv_feature = decoded["mv_feature"].permute(0, 2, 3, 1)
            out_dec, out_dec_c = self._decompress_files_end(begun)
            torch.cuda.synchronize()
            decoding_time = time.time() - t0
            luma = dict(luma, H_t_hat=out_dec["H_t"]["x_hat"], L_t_hat=out_dec["L_t"]["x_hat"] if code_lt else None)
            chroma = dict(chroma, H_t_hat=out_dec_c["H_t"]["x_hat"],
                          L_t_hat=out_dec_c["L_t"]["x_hat"] if code_lt else None)
        result = {
            "L_t": luma["L_t_hat"] if code_lt else luma["L_t"],
            "H_t": luma["H_t_hat"],
            "L_tc": chroma["L_t_hat"] if code_lt else chroma["L_t"],
            "H_tc": chroma["H_t_hat"],
            "bit_H": bits["H"] + bits["Hc"],
            "bit_L": bits["L"] + bits["Lc"] if code_lt else None,
            "bit_Lc": bits["Lc"] if code_lt else None,
            "bit_Hc": bits["Hc"],
            "bit_ME": bits["mv"],
            "mv_hat": mv_hat,
            "dpb": {"mv_feature": mv_feature.permute(0, 3, 1, 2), "ref_mv_y": mv["mv_y_hat"].permute(0, 3, 1, 2)},
            "decoding_time": decoding_time,
            "encoding_time": encoding_time,
        }
        if keep:
            result["files"] = {k: v[1] for k, v in done.items()}
            result["traces"] = {k: v[2] for k, v in done.items()}
        if relayed and torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_backend() == "nccl":
            # the context of this pair travels over RCCL, whose watchdog thread queries events at any moment: no stream
            # capture beside it (a plan recorded earlier, e.g. by bench.py's GOP-level phase, is still replayed)
            plan_key = None
        if plan_key is not None and eng.use_graphs and len(eng.host_threads) <= 1:
            # every layer of this configuration is packed now: record its launches, the next such pair replays them
            from pMCTF.hip.pair_plan import PairPlan
            try:
                with eng.gate.exclusive_from_shared():
                    torch.cuda.synchronize(dev)
                    eng.pair_plans[plan_key] = PairPlan(eng, ref_y, ref_chroma, plan_key[3], bool(code_lt), stage_idx,
                                                        q_index, me_downsample)
            except Exception as e:  # noqa: BLE001 - recording is an optimisation: keep coding through stream launches
                import warnings
                warnings.warn(f"pMCTF: recording the launch plan failed ({type(e).__name__}: {e}); this engine goes on "
                              f"with stream launches (same results)")
                eng.use_graphs = False
        return result

    def _encode_pair_planned(self, plan, ry, cy, rc, cc, code_lt, dpb, output_path, pic_width, pic_height, on_dpb):
        """encode_one_stage's write branch (skip_decoding) through a captured launch plan (pMCTF.hip.pair_plan): same
        kernels, files, bits and tensors as the stream path; luma and chroma coders run concurrently."""
        eng = self.engine()
        start = time.time()
        keep = eng.keep_streams
        base = osp.basename(output_path)
        paths = {"mv": output_path.replace(".bin", "_mv.bin"), "H": output_path,
                 "Hc": output_path.replace(".bin", "_C_main.bin"), "L": output_path.replace(base, "0_main.bin"),
                 "Lc": output_path.replace(base, "0_C_main.bin")}
        headers = {"mv": lambda n: mv_header(n, 0)}
        for k in ("H", "L"):
            headers[k] = lambda n: image_header(pic_height, pic_width, 1, n)
            headers[k + "c"] = lambda n: image_header(pic_height // 2, pic_width // 2, 2, n)
        jobs = {}

        def submit(job, hs, hi, ev, segments):
            jobs[job] = eng.coder.submit_host(hs, hi, ev, segments, eng.tables, headers[job], paths[job], keep)
        if not callable(dpb):
            dpb = unwrap(dpb)
        r = plan.run(eng, ry, cy, rc, cc, dpb, submit, on_dpb)
        t_enq = time.time() - start
        done = {k: j.result() for k, j in jobs.items()}
        eng.stats["enqueue_s"] += t_enq
        eng.stats["pair_s"] += time.time() - start
        eng.stats["pairs"] += 1
        bits = {k: v[0] * 8.0 for k, v in done.items()}
        result = {"L_t": r["L_t"], "H_t": r["H_t"], "L_tc": r["L_tc"], "H_tc": r["H_tc"],
                  "bit_H": bits["H"] + bits["Hc"], "bit_L": bits["L"] + bits["Lc"] if code_lt else None,
                  "bit_Lc": bits["Lc"] if code_lt else None, "bit_Hc": bits["Hc"], "bit_ME": bits["mv"],
                  "mv_hat": r["mv_hat"],
                  "dpb": {"mv_feature": r["mv_feature"].permute(0, 3, 1, 2), "ref_mv_y": r["mv_y_hat"].permute(0, 3, 1, 2)},
                  "decoding_time": 0, "encoding_time": time.time() - start}
        if keep:
            result["files"] = {k: v[1] for k, v in done.items()}
            result["traces"] = {k: v[2] for k, v in done.items()}
        return result
