"""Cases of the direct tests of the bf16-split 3x3 convolution (csrc/conv_split.hip), their expected values from
tests/split_restatement.py, and the code that runs them on the GPU.  Used by tests/test_gpu_split_conv.py in process
(the kernel the dispatcher picks) and as a child process for the kernel variants that PMCTF_SPLIT_VARIANT forces (the
variable is read once per process):

    PMCTF_SPLIT_VARIANT=<0|1|2> python split_conv_helper.py <variant> out.npz

tests/test_split_restatement_cpu.py imports the case list from here, so the conditions it checks on the exact data are
checked on the very inputs the GPU sees.  Importing this module needs neither the product nor a GPU.

Entry points of conv_split.hip and where they are reached:
    pmctf_conv3x3_split_supported, pmctf_conv3x3_split_packed_size, pmctf_conv3x3_split_pack_weights
                                    ops.Conv2d(..., split=ns) below; the packing itself bit for bit in the CPU test
    pmctf_conv3x3_split_f32         ops.Conv2d.__call__ with ops.SPLIT_MIN_PX = 0: the stride-1 cases
    pmctf_conv3x3_split_geom_f32    ops.conv_at_class: the stride-2 cases, all four parity classes
"""
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "learned-pmctf_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import split_restatement as sr  # noqa: E402

SWITCH = "PMCTF_SPLIT_VARIANT"
VARIANTS = (0, 1, 2)            # workgroup kernel with LDS-shared fragments / wave kernel, two workgroups per CU / one
NSPLITS = (1, 2, 3)
EPILOGUES = [(act, slope, nres) for act, slope in ((0, 0.0), (1, 0.0), (2, 0.2)) for nres in (0, 1, 2)]

Case = collections.namedtuple("Case", "name N Cin Cout H W stride seed")

# The smallest shapes that reach every boundary of the 16x32 (variant 0) and 8x32 workgroup tiles, the 4x16 wave tile,
# the 16-channel chunk loop and the batch axis.  (N, Cin, Cout, H, W)
STRIDE1 = [
    (1, 16, 64, 3, 5),          # less than one wave tile; a single chunk: no fetch(cb + 1), one LDS stage for KBPS = 5
    (1, 16, 112, 16, 32),       # exactly one variant-0 tile
    (2, 32, 64, 19, 37),        # ragged on both axes, two chunks, two planes
    (1, 112, 112, 9, 70),       # seven chunks x seven cout tiles; the third tile column is 6 px wide
    (3, 64, 112, 33, 17),       # the second wave column holds one pixel; one row past two tiles
    (1, 112, 64, 8, 33),        # seven chunks x four cout tiles; one pixel past a tile column
]
# stride 2, 112 couts, every parity class: (N, Cin, H, W)
STRIDE2 = [(1, 16, 2, 2), (2, 32, 18, 70), (1, 112, 34, 38)]

CASES = ([Case(f"s1_{n}x{ci}x{co}x{h}x{w}", n, ci, co, h, w, 1, 100 + k) for k, (n, ci, co, h, w) in enumerate(STRIDE1)]
         + [Case(f"s2_{n}x{ci}x{h}x{w}", n, ci, 112, h, w, 2, 200 + k) for k, (n, ci, h, w) in enumerate(STRIDE2)])
STRIDE1_CASES = [c for c in CASES if c.stride == 1]


def geometries(c):
    """[(tag, parity class or None, keyword arguments of the restatement)]"""
    if c.stride == 1:
        return [("full", None, dict(stride=1, pad=(1, 1), out_hw=(c.H, c.W)))]
    return [(f"class{cls}", cls, dict(stride=2, pad=(1 - (cls >> 1), 1 - (cls & 1)), out_hw=(c.H // 2, c.W // 2)))
            for cls in range(4)]


def inputs(c, kind):
    """(x NHWC, w OIHW, b) of case c: kind "exact" or "dense" """
    make = {"exact": sr.exact_case, "dense": sr.dense_case}[kind]
    return make(c.N, c.Cin, c.Cout, c.H, c.W, c.seed + (0 if kind == "exact" else 1000))


def case_residuals(c):
    ho, wo = geometries(c)[0][2]["out_hw"]
    return sr.residuals((c.N, ho, wo, c.Cout), c.seed + 2000)


def key(c, kind, tag, ns, epi=EPILOGUES[0]):
    return f"{c.name}__{kind}__{tag}__ns{ns}__act{epi[0]}res{epi[2]}"


def instantiation(variant, cout, ns, stride=1):
    """the template instance a launch ends in (mirror of dispatch_ns and the two entry points); variant None: the
    dispatcher's own choice"""
    mt = cout // 16
    if stride == 2:
        return f"launch_split_wave<7, {ns}, 1, 2>"
    if variant is None:
        variant = 2 if (ns == 2 and mt == 7) or (ns == 3 and mt == 4) else 1
    if variant == 0:
        return f"launch_split<{mt}, {ns}, {5 if ns == 1 else 1}>"
    return f"launch_split_wave<{mt}, {ns}, {2 if variant == 1 else 1}>"


# --------------------------------------------------------------------------------------------- expected, on the CPU
def expected_exact(c):
    """{key: float32 output the kernel must produce bit for bit} for every geometry, ns and epilogue of case c, and
    {(tag, ns): (S, A)}"""
    x, w, b = inputs(c, "exact")
    res = case_residuals(c)
    want, sums = {}, {}
    for tag, _, g in geometries(c):
        for ns in NSPLITS:
            S, A = sr.conv_ref(x, w, b, ns, **g)
            sums[(tag, ns)] = (S, A)
            v = S.astype(np.float32)
            for epi in EPILOGUES:
                want[key(c, "exact", tag, ns, epi)] = sr.epilogue(v, epi[0], epi[1], res[:epi[2]])
    return want, sums


def expected_dense(c):
    """{key: (S, T, C, E)}: the restatement's sum, the accumulation bound, the float64 convolution of the unsplit operands
    and EPS[ns] * sum |x||w|"""
    x, w, b = inputs(c, "dense")
    out = {}
    for tag, _, g in geometries(c):
        C64, B = sr.conv64(x, w, b, **g)
        for ns in NSPLITS:
            S, A = sr.conv_ref(x, w, b, ns, **g)
            out[key(c, "dense", tag, ns)] = (S, sr.accumulation_bound(A, c.Cin, ns), C64, sr.EPS[ns] * B)
    return out


# ------------------------------------------------------------------------------------------------------ on the GPU
def run(cases, log=None):
    """every case in `cases` through ops.Conv2d(split=ns) / ops.conv_at_class on cuda:0, each launch twice:
    ({key: output}, {key: the two launches gave equal bits})"""
    import torch
    from pMCTF.hip import ops
    dev = torch.device("cuda:0")
    out, same = {}, {}
    old = ops.SPLIT_MIN_PX
    ops.SPLIT_MIN_PX = 0
    try:
        for c in cases:
            t0 = time.time()
            res = [torch.from_numpy(r).to(dev) for r in case_residuals(c)]
            for kind in ("exact", "dense"):
                x, w, b = inputs(c, kind)
                xt = torch.from_numpy(x).to(dev)
                for ns in NSPLITS:
                    conv = ops.Conv2d(torch.from_numpy(w), torch.from_numpy(b), 1, (1, 1), split=ns)
                    assert conv.split == ns, f"{c.name}: no split kernel for this shape"
                    for tag, cls, _ in geometries(c):
                        for epi in (EPILOGUES if kind == "exact" else EPILOGUES[:1]):
                            kw = dict(act=epi[0], slope=epi[1], res1=res[0] if epi[2] > 0 else None,
                                      res2=res[1] if epi[2] > 1 else None)
                            ys = [conv(xt, **kw) if cls is None else ops.conv_at_class(conv, xt, cls, **kw)
                                  for _ in range(2)]
                            k = key(c, kind, tag, ns, epi)
                            out[k] = ys[0].cpu().numpy()
                            same[k] = bool(torch.equal(ys[0], ys[1]))
            if log:
                log(f"{c.name}: {time.time() - t0:.2f} s")
    finally:
        ops.SPLIT_MIN_PX = old
    return out, same


def main():
    variant, path = sys.argv[1:3]
    assert os.environ.get(SWITCH) == variant and int(variant) in VARIANTS, f"{SWITCH} must be set to {variant}"
    out, same = run(STRIDE1_CASES)
    np.savez(path, **out, **{"same__" + k: np.array(v) for k, v in same.items()})


if __name__ == "__main__":
    main()
