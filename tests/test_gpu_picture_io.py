"""Picture input / output kernels on the GPU (csrc/picture_ops.hip through pMCTF.hip.ops.frame_to_rgb8 / planes_from_u8 /
rgb8_to_yuv420, pmctf_gop.frames_to_rgb8 / read_gop_device / pngs_to_yuv / encode_sequence / decode_sequence and the two
command-line tools).

Every expectation is a torch statement on CPU tensors, equal byte for byte: the harness's own statements
(tests/quality_restatement.py: harness_pictures) for the RGB pictures, pmctf_gop.read_gop on the CPU for the model's
inputs, and the formulas of rgb2ycbcr (pMCTF/utils/util.py:21-40) written out below for the RGB -> 4:2:0 converter."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_restatement as qr
from helpers import product_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- 1. RGB out
def _expected_rgb8(rec_y, rec_c, h, w):
    """CPU float32 planes -> ((h, w, 3) uint8 array, the rounded RGB picture before the clip)"""
    zero_y, zero_c = torch.zeros((1, 1, h, w)), torch.zeros((2, 1, h // 2, w // 2))
    raw = qr.harness_pictures(rec_y, rec_c, zero_y, zero_c, h, w)[2]
    return raw.clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous().numpy(), raw


def _reconstruction(Hp, Wp, h, w):
    """uniform in [-40, 300] on the padded planes; over the first rows of each plane's crop exact k + 0.5 values spread
    from -1.5 to 257.5"""
    g = torch.Generator().manual_seed(Hp * 7 + Wp * 5 + h * 3 + w)
    rec_y = torch.rand((1, 1, Hp, Wp), generator=g) * 340.0 - 40.0
    rec_c = torch.rand((2, 1, Hp // 2, Wp // 2), generator=g) * 340.0 - 40.0
    halves = torch.arange(-2, 258, dtype=torch.float32) + 0.5
    for plane, rows, cols in ((rec_y[0, 0], h, w), (rec_c[0, 0], h // 2, w // 2), (rec_c[1, 0], h // 2, w // 2)):
        k, n = min(cols, 52), min(rows, 5)
        pick = torch.linspace(0, halves.numel() - 1, k * n).round().long()
        plane[:n, :k] = halves[pick].view(n, k)
    return rec_y, rec_c


@pytest.mark.parametrize("Hp,Wp,h,w", [(128, 128, 2, 2), (128, 128, 18, 22), (128, 256, 100, 132), (256, 384, 130, 258)])
def test_frame_to_rgb8_equals_the_harness_statements(cuda, Hp, Wp, h, w):
    from pMCTF.hip import ops
    rec_y, rec_c = _reconstruction(Hp, Wp, h, w)
    want, raw = _expected_rgb8(rec_y, rec_c, h, w)
    # premises, on the CPU side
    crop = rec_y[0, 0, :h, :w]
    assert float(crop.min()) < 0.0 and float(crop.max()) > 255.0, "the clamp of luma is live inside the crop"
    inside = crop[(crop > 0) & (crop < 255)]
    assert bool(((inside % 1.0) == 0.5).any()), "an exact tie inside the crop and inside the clamp"
    for c in (rec_c[0, 0, :h // 2, :w // 2], rec_c[1, 0, :h // 2, :w // 2]):
        assert bool(((c % 1.0) == 0.5).any()), "an exact tie inside the crop of each chroma plane"
    assert bool((raw < 0).any()) and bool((raw > 255).any()), "the final clip changes a value at each end"
    assert want.shape == (h, w, 3) and want.dtype == np.uint8

    got = ops.frame_to_rgb8(rec_y.to(cuda), rec_c.to(cuda), h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.is_cuda and got.is_contiguous()
    diff = np.argwhere(got.cpu().numpy() != want)
    assert diff.size == 0, f"{len(diff)} bytes differ, first at (y, x, channel) {diff[0]}"
    again = ops.frame_to_rgb8(rec_y.to(cuda), rec_c.to(cuda), h, w)
    assert torch.equal(again, got)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = ops.frame_to_rgb8(rec_y.to(cuda), rec_c.to(cuda), h, w)
    s.synchronize()
    assert torch.equal(side, got)


# ---------------------------------------------------------------------------------------------------- 2. bytes in
@pytest.mark.parametrize("psize", [128, 256])
@pytest.mark.parametrize("h,w", [(6, 10), (18, 22), (100, 132), (128, 128)])
def test_planes_from_u8_equals_read_gop_on_the_cpu(cuda, tmp_path, h, w, psize):
    import pmctf_gop
    from pMCTF.hip import ops
    from pMCTF.utils.yuv_reader import YUVReader
    rng = np.random.default_rng(h * 1000 + w)
    frame = rng.integers(0, 256, h * w * 3 // 2, dtype=np.uint8)
    if (h, w) == (6, 10):
        assert (h * w + (h // 2) * (w // 2)) % 2 == 1, "the Cr plane starts at an odd byte"
    path = str(tmp_path / "one.yuv")
    frame.tofile(path)
    reader = YUVReader(path, w, h)
    padded, orig, size = pmctf_gop.read_gop(reader, 1, "cpu", psize)
    reader.close()
    assert size == (h, w)
    got = ops.planes_from_u8(torch.from_numpy(frame).to(cuda), h, w, psize=psize)
    want = (padded[0][0], padded[0][1], orig[0][0], orig[0][1])
    for name, a, b in zip(("y_pad", "c_pad", "y_org", "c_org"), got, want):
        assert a.dtype == torch.float32 and a.is_cuda and a.is_contiguous() and tuple(a.shape) == tuple(b.shape), name
        assert torch.equal(a.cpu(), b), name
    Hp, Wp = got[0].shape[-2:]
    assert Hp % psize == 0 and Wp % psize == 0 and ((Hp, Wp) == (h, w)) == ((h, w) == (128, 128) and psize == 128)
    only = ops.planes_from_u8(torch.from_numpy(frame).to(cuda), h, w, psize=psize, originals=False)
    assert only[2] is None and only[3] is None
    assert torch.equal(only[0], got[0]) and torch.equal(only[1], got[1])


GUARD = 64                                            # floats / bytes on either side of every guarded output


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _guarded(numel, np_dtype, dev, fill, offset=0):
    """(whole buffer, the view of numel elements that starts GUARD + offset elements in)"""
    buf = torch.from_numpy(np.full(numel + 2 * GUARD + offset, fill, dtype=np_dtype)).to(dev)
    return buf, buf[GUARD + offset:GUARD + offset + numel]


def _guards_untouched(buf, numel, fill, offset=0):
    host = buf.cpu().numpy()
    return bool((host[:GUARD + offset] == fill).all()) and bool((host[GUARD + offset + numel:] == fill).all())


@pytest.mark.parametrize("h,w,psize", [(6, 10, 2), (10, 6, 2), (18, 34, 16), (100, 132, 128)])
def test_ingest_equals_read_gop_at_every_source_alignment(cuda, tmp_path, h, w, psize):
    """the 8-bit sibling of test_gpu_high_bitdepth.py::test_ingest_equals_the_restatement_at_every_source_alignment: the
    source 0..3 bytes past a multiple of 4, with and without originals, every output between guards"""
    import pmctf_gop
    from pMCTF.hip import lib
    from pMCTF.utils.yuv_reader import YUVReader
    rng = np.random.default_rng(h * 1000 + w)
    frame = rng.integers(0, 256, h * w * 3 // 2, dtype=np.uint8)
    frame[0], frame[1], frame[h * w], frame[-1] = 0, 255, 255, 0
    if (h, w) == (6, 10):
        assert (h * w + (h // 2) * (w // 2)) % 2 == 1, "the Cr plane starts at an odd byte"
    path = str(tmp_path / "one.yuv")
    frame.tofile(path)
    reader = YUVReader(path, w, h)
    padded, orig, _ = pmctf_gop.read_gop(reader, 1, "cpu", psize)
    reader.close()
    want = [t.numpy() for t in (padded[0][0], padded[0][1], orig[0][0], orig[0][1])]
    Hp, Wp = want[0].shape[-2:]
    if (h, w, psize) == (18, 34, 16):
        assert w % 4 == 2 and (Hp, Wp) == (32, 48), "rows of w % 4 = 2 bytes against padded rows of whole groups"
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fill = -7.0
    for off in range(4):
        big = torch.from_numpy(np.concatenate((np.zeros(off, np.uint8), frame, np.zeros(4 - off, np.uint8)))).to(cuda)
        assert big.data_ptr() % 4 == 0
        src = big[off:off + frame.size]
        assert src.data_ptr() % 4 == off
        for with_org in (True, False):
            bufs = [_guarded(e.size, np.float32, cuda, fill) for e in want]
            views = [v for _, v in bufs]
            assert all(v.data_ptr() % 16 == 0 for v in views[:2])
            rc = L.pmctf_yuv420_u8_to_planes_f32(_ptr(src), _ptr(views[0]), _ptr(views[1]),
                                                 _ptr(views[2]) if with_org else None,
                                                 _ptr(views[3]) if with_org else None, Hp, Wp, h, w, stream)
            assert rc == 0
            for k, ((buf, v), e) in enumerate(zip(bufs, want)):
                if k < 2 or with_org:
                    got = v.cpu().numpy().reshape(e.shape)
                    diff = np.argwhere(got.view(np.uint32) != e.view(np.uint32))
                    assert diff.size == 0, (off, with_org, k, diff[0], got[tuple(diff[0])], e[tuple(diff[0])])
                else:
                    assert bool((v.cpu().numpy() == fill).all()), "null originals: nothing written"
                assert _guards_untouched(buf, e.size, fill), (off, with_org, k)


def _planes_with_specials(N, Hp, Wp, h, w):
    """as _reconstruction of test_gpu_high_bitdepth.py at 8 bits: uniform in [-40, 300]; inside the crop NaN, +-inf, -0.0,
    the values around 255 and exact ties k + 0.5"""
    g = torch.Generator().manual_seed(N * 11 + Hp * 7 + Wp * 5 + h * 3 + w)
    x = torch.rand((N, 1, Hp, Wp), generator=g) * 340.0 - 40.0
    special = [float("nan"), float("inf"), float("-inf"), -0.0, 255.0, float(np.nextafter(np.float32(255), np.float32(1e9))),
               256.0, 0.5, 1.5, 2.5, -0.5, 254.5, 255.5]
    ties = [k + 0.5 for k in np.linspace(3, 252, 40).astype(np.int64)]
    vals = torch.tensor(special + ties, dtype=torch.float32)
    for n in range(N):
        flat_idx = torch.randperm(h * w, generator=g)[:min(len(vals), h * w)]
        x[n, 0, flat_idx // w, flat_idx % w] = vals[:len(flat_idx)]
    return x


@pytest.mark.parametrize("N,Hp,Wp,h,w", [(2, 3, 5, 3, 5), (3, 8, 8, 5, 1), (1, 4, 4, 4, 4), (2, 32, 48, 18, 34),
                                         (1, 32, 48, 18, 35), (2, 66, 130, 65, 129)])
def test_output_at_every_destination_alignment(cuda, N, Hp, Wp, h, w):
    """pmctf_planes_to_u8 with out 0..3 bytes past a multiple of 4, guard bytes on both sides: NaN -> 0, then
    rint(clip(x, 0, 255)), written out in numpy"""
    from pMCTF.hip import lib, ops
    x = _planes_with_specials(N, Hp, Wp, h, w)
    crop = x[:, 0, :h, :w].numpy()
    want = np.rint(np.clip(np.where(np.isnan(crop), np.float32(0), crop), 0, 255)).astype(np.uint8)
    if h * w > 60:
        assert np.isnan(crop).any() and np.isinf(crop).any() and (crop[np.isfinite(crop)] % 1.0 == 0.5).any()
        assert np.signbit(crop[crop == 0]).any() and crop[np.isfinite(crop)].min() < 0 and crop[np.isfinite(crop)].max() > 255
    if (N, h, w) == (2, 3, 5):
        assert w % 4 == 1 and (N * h * w) % 4 == 2, "rows of w % 4 = 1 bytes, two tail bytes"
    xd = x.to(cuda)
    got = ops.planes_to_u8(xd, h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, h, w) and got.is_cuda and got.is_contiguous()
    diff = np.argwhere(got.cpu().numpy() != want)
    assert diff.size == 0, f"{len(diff)} bytes differ, first at (n, y, x) {diff[0]}"
    L = lib.hip()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in range(4):
        buf, view = _guarded(N * h * w, np.uint8, cuda, 0xA5, offset=off)
        assert view.data_ptr() % 4 == off
        assert L.pmctf_planes_to_u8(_ptr(xd), _ptr(view), N, Hp, Wp, h, w, stream) == 0
        assert np.array_equal(view.cpu().numpy().reshape(N, h, w), want), off
        assert _guards_untouched(buf, N * h * w, 0xA5, offset=off), off


def test_read_gop_device_equals_read_gop(cuda, tmp_path):
    import pmctf_gop
    import pmctf_synth
    from pMCTF.utils.yuv_reader import YUVReader
    w, h, n = 22, 18, 3
    path = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(path, pmctf_synth.synth_yuv420(w, h, n, seed=3))
    for psize in (128, 2):                           # 2: nothing to pad, as sequence_quality reads its files
        r = YUVReader(path, w, h)
        want = pmctf_gop.read_gop(r, n, "cpu", psize)
        r.close()
        r = YUVReader(path, w, h)
        got = pmctf_gop.read_gop_device(r, n, cuda, psize)
        r.close()
        assert got[2] == want[2] == (h, w)
        for k in range(n):
            for part in (0, 1):
                for a, b in zip(got[part][k], want[part][k]):
                    assert a.is_cuda and a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
                    assert torch.equal(a.cpu(), b), (psize, k, part)


# ---------------------------------------------------------------------------------------------------- 3. RGB in
def _yuv420_of_rgb_cpu(rgb):
    """(h, w, 3) uint8 CPU tensor -> uint8 tensor of h*w*3/2: rgb2ycbcr in float32 in its written order, the 2x2 chroma sum
    in the stated order, round half to even of the clamp.  Also returns the unrounded luma."""
    r, g, b = rgb[:, :, 0].float(), rgb[:, :, 1].float(), rgb[:, :, 2].float()
    y = 0.299 * r + 0.587 * g + 0.114 * b
    cb = (b - y) * 0.564 + 128.0
    cr = (r - y) * 0.713 + 128.0
    assert y.dtype == torch.float32 and cb.dtype == torch.float32
    mean = lambda c: (((c[0::2, 0::2] + c[0::2, 1::2]) + c[1::2, 0::2]) + c[1::2, 1::2]) * 0.25
    planes = [torch.round(p.clamp(0, 255)).to(torch.uint8).reshape(-1) for p in (y, mean(cb), mean(cr))]
    return torch.cat(planes), y


_ties = {}


def _tie_colours():
    """colours whose luma is exactly k + 0.5 in float32, from R, G in 0..255, B in 0, 5, .., 255"""
    if "c" not in _ties:
        r, g, b = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), torch.arange(0.0, 256.0, 5.0), indexing="ij")
        y = 0.299 * r + 0.587 * g + 0.114 * b
        at = (y - torch.floor(y)) == 0.5
        _ties["c"] = torch.stack((r[at], g[at], b[at]), dim=1).to(torch.uint8)
    return _ties["c"]


@pytest.mark.parametrize("h,w", [(2, 2), (6, 10), (18, 22), (100, 132)])
def test_rgb8_to_yuv420_equals_the_written_formulas(cuda, h, w):
    from pMCTF.hip import ops
    ties = _tie_colours()
    assert len(ties) >= 4, "luma ties exist in float32"
    g = torch.Generator().manual_seed(h * 1000 + w)
    rgb = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    pick = ties[torch.linspace(0, len(ties) - 1, 4).long()]
    rgb.view(-1, 3)[:4] = pick                      # the first pixels of the first row (all four pixels of the 2x2 picture)
    want, y = _yuv420_of_rgb_cpu(rgb)
    assert bool(((y - torch.floor(y)) == 0.5).any()), "the picture holds a luma tie"
    got = ops.rgb8_to_yuv420(rgb.to(cuda))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h * w * 3 // 2,) and got.is_cuda
    diff = torch.nonzero(got.cpu() != want)
    assert diff.numel() == 0, f"{len(diff)} bytes differ, first at byte {int(diff[0])} of {want.numel()} (luma: {h * w})"
    assert torch.equal(ops.rgb8_to_yuv420(rgb.to(cuda)), got)


def test_greys_map_to_neutral_chroma(cuda):
    from pMCTF.hip import ops
    v = torch.arange(256, dtype=torch.uint8)
    rgb = v.view(1, 256, 1).expand(2, 256, 3).contiguous()            # two rows of the 256 greys
    got = ops.rgb8_to_yuv420(rgb.to(cuda)).cpu()
    assert torch.equal(got[:512], torch.cat((v, v)))
    assert torch.equal(got[512:], torch.full((256,), 128, dtype=torch.uint8))
    assert torch.equal(_yuv420_of_rgb_cpu(rgb)[0], got)


# ---------------------------------------------------------------------------------------------------- 4 - 6. the drivers
W, H, GOP, Q = 96, 112, 2, 3                         # pads to 128x128


@pytest.fixture(scope="module")
def net(cuda):
    return product_model(1)[0]


def _files(folder):
    """{relative path: bytes} of every file below folder, without the header's text (compared on its own)"""
    out = {}
    for base, _, names in os.walk(folder):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def _read_pngs(folder, count):
    from PIL import Image
    assert sorted(os.listdir(folder), key=lambda n: int(n[:-4])) == [f"{i}.png" for i in range(count)]
    pics = []
    for i in range(count):
        im = Image.open(os.path.join(folder, f"{i}.png"))
        assert im.mode == "RGB" and im.size == (W, H)
        pics.append(np.asarray(im))
    return pics


def test_decoded_pictures_as_pngs(cuda, net, tmp_path):
    import pmctf_gop
    import pmctf_synth
    src = str(tmp_path / "src.yuv")
    pmctf_gop.write_yuv(src, pmctf_synth.synth_yuv420(W, H, GOP, seed=21))
    bins, enc_png = str(tmp_path / "bins"), str(tmp_path / "enc_png")
    os.makedirs(bins)
    pmctf_gop.encode_sequence(net, src, W, H, GOP, GOP, Q, bins, "cuda", keep_gops=True, decoded_frame_path=enc_png)
    assert sorted(os.listdir(bins)) == ["gop_00000", "sequence.json"]
    assert sorted(os.listdir(os.path.join(bins, "gop_00000"))) == sorted(pmctf_gop.gop_file_names(GOP))

    dec_net = product_model(1)[0]
    plain, both, png = str(tmp_path / "plain.yuv"), str(tmp_path / "both.yuv"), str(tmp_path / "png")
    pmctf_gop.decode_sequence(dec_net, bins, plain, "cuda")
    res = pmctf_gop.decode_sequence(dec_net, bins, both, "cuda", png_out=png)
    assert res["frames"] == [(H, W)] * GOP
    assert open(both, "rb").read() == open(plain, "rb").read()
    only = str(tmp_path / "only_png")
    res = pmctf_gop.decode_sequence(dec_net, bins, None, "cuda", png_out=only)
    assert res["frames"] == [(H, W)] * GOP
    with pytest.raises(ValueError):
        pmctf_gop.decode_sequence(dec_net, bins, None, "cuda")

    frames = pmctf_gop.decode_gop_files(dec_net, os.path.join(bins, "gop_00000"), GOP, H, W, Q)["frames"]
    direct = pmctf_gop.frames_to_rgb8(frames, H, W)
    got, got_only, got_enc = _read_pngs(png, GOP), _read_pngs(only, GOP), _read_pngs(enc_png, GOP)
    for i, (ry, rc, _) in enumerate(frames):
        want, _ = _expected_rgb8(ry.cpu(), rc.cpu(), H, W)
        assert direct[i].dtype == np.uint8 and np.array_equal(direct[i], want), i
        assert np.array_equal(got[i], want) and np.array_equal(got_only[i], want), i
        assert np.array_equal(got_enc[i], want), f"frame {i}: the encoder side's decoded_frame_path picture differs"


@pytest.fixture(scope="module")
def png_source(tmp_path_factory):
    import pmctf_gop
    folder = str(tmp_path_factory.mktemp("picture_io") / "src_png")
    rng = np.random.default_rng(17)
    # smooth ramps plus noise, so that neither the coder nor the colour conversion sees a flat picture
    yy, xx = np.mgrid[0:H, 0:W]
    pics = []
    for k in range(GOP):
        base = np.stack(((2 * xx + k) % 256, (2 * yy + 3 * k) % 256, (xx + yy) % 256), axis=2)
        pics.append(np.clip(base + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8))
    pmctf_gop.write_pngs(folder, 0, pics)
    return folder, pics


def test_png_source_codes_like_its_yuv(cuda, net, png_source, tmp_path):
    import pmctf_gop
    folder, pics = png_source
    a, b, c = (str(tmp_path / n) for n in "abc")
    for d in (a, b, c):
        os.makedirs(d)
    ra = pmctf_gop.encode_sequence(net, folder, W, H, GOP, GOP, Q, a, "cuda", keep_gops=True, src_format="png")
    yuv = str(tmp_path / "from_png.yuv")
    assert pmctf_gop.pngs_to_yuv(folder, yuv, "cuda") == (W, H, GOP)
    data = np.fromfile(yuv, dtype=np.uint8)
    assert data.size == GOP * W * H * 3 // 2
    for k in range(GOP):
        want, _ = _yuv420_of_rgb_cpu(torch.from_numpy(pics[k]))
        assert np.array_equal(data[k * W * H * 3 // 2:(k + 1) * W * H * 3 // 2], want.numpy()), k
    rb = pmctf_gop.encode_sequence(net, yuv, W, H, GOP, GOP, Q, b, "cuda", keep_gops=True)
    rc = pmctf_gop.encode_sequence(net, yuv, W, H, GOP, GOP, Q, c, "cuda", keep_gops=True, ingest="device")
    fa, fb, fc = _files(a), _files(b), _files(c)
    assert sorted(fa) == sorted(fb) == sorted(fc) and len(fa) == 1 + len(pmctf_gop.gop_file_names(GOP))
    for name in fa:
        assert fa[name] == fb[name], f"{name}: PNG source against its .yuv"
        assert fc[name] == fb[name], f"{name}: device ingest against host ingest"
    for other in (ra, rc):
        for k in ("bits", "psnr", "psnr_rgb", "bpp_mv", "frame_types"):
            assert other[k] == rb[k], k
    with pytest.raises(ValueError, match="not"):
        pmctf_gop.encode_sequence(net, folder, W + 2, H, GOP, GOP, Q, a, "cuda", src_format="png")
    for kw in ({"src_format": "png"}, {"ingest": "device"}):
        with pytest.raises(RuntimeError):
            pmctf_gop.encode_sequence(net, folder if "src_format" in kw else yuv, W, H, GOP, GOP, Q, a, "cpu", **kw)


def test_encode_and_decode_tools(cuda, png_source, tmp_path):
    folder, _ = png_source
    bins, enc_png, dec_png = str(tmp_path / "bins"), str(tmp_path / "enc_png"), str(tmp_path / "dec_png")
    enc = [sys.executable, os.path.join(ROOT, "tools", "encode_sequence.py"), "--synth-seed", "0", "--gop", str(GOP),
           "--q-index", str(Q), "--decoded-frames", enc_png, folder, bins]
    r = subprocess.run(enc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    record = json.loads(r.stdout[r.stdout.index("{"):])
    assert record["frame_pixel_num"] == W * H and len(record["frame_bpp"]) == GOP and record["i_frame_num"] == 1
    assert sorted(os.listdir(bins)) == ["gop_00000", "sequence.json"]
    dec = [sys.executable, os.path.join(ROOT, "tools", "decode_sequence.py"), "--synth-seed", "0", "--png", dec_png, bins]
    r = subprocess.run(dec, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["width"], summary["height"], summary["yuv"]) == (GOP, W, H, None)
    a, b = _read_pngs(enc_png, GOP), _read_pngs(dec_png, GOP)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    r = subprocess.run(dec[:-3] + [bins], capture_output=True, text=True, timeout=600)     # nothing to write
    assert r.returncode != 0
