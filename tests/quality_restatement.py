"""Yardsticks of the quality-metric tests, in plain torch on whatever device and dtype the caller picks.

MS-SSIM is restated from the published definition (Wang, Simoncelli, Bovik: "Multiscale structural similarity for image
quality assessment", 2003) with the defaults the evaluation harness gets from ms_ssim(x, y, data_range=255.0): five scales,
weights 0.0448 / 0.2856 / 0.3001 / 0.2363 / 0.1333, an 11-tap Gaussian window (sigma 1.5, normalised to sum 1) applied
separably without padding, C1 = (0.01*255)^2, C2 = (0.03*255)^2, a 2x2 average pool (stride 2, zero padding of size % 2,
the padding counted in the average) between scales, relu before the powers, mean over the channels.  The package itself
is on none of the machines this project runs on, so it cannot be the pin; the float64 run of this file on the CPU is.

The PSNR yardstick is the harness's own sequence of torch calls (round(clamp), crop, yuv_420_to_444, ycbcr2rgb, round) on
CPU tensors, with the squared-error sums taken in int64."""
import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN_SIZE, WIN_SIGMA = 11, 1.5
MIN_SIDE = (WIN_SIZE - 1) * 2 ** (len(WEIGHTS) - 1)            # 160: the smaller side must exceed it
# the GPU tests' pictures: (Hp, Wp, h, w) and the standard deviation of the noise added to the original
CASES = ((1088, 1920, 1080, 1920), (128, 256, 100, 132), (384, 640, 360, 636), (256, 256, 192, 256))
NOISE = (0.4, 3.0, 25.0)


def gauss_window(dtype):
    coords = torch.arange(WIN_SIZE, dtype=dtype) - WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * WIN_SIGMA ** 2))
    return g / g.sum()


def _blur(x, win):
    """separable, no padding: (N,C,H,W) -> (N,C,H-10,W-10)"""
    C = x.shape[1]
    x = F.conv2d(x, win.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(x, win.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)


def scale_means(x, y, win, data_range=255.0):
    """-> (mean cs, mean ssim) per channel, each of shape (C,), for N = 1"""
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu1, mu2 = _blur(x, win), _blur(y, win)
    s11 = _blur(x * x, win) - mu1 * mu1
    s22 = _blur(y * y, win) - mu2 * mu2
    s12 = _blur(x * y, win) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs
    return cs.flatten(2).mean(-1)[0], ssim.flatten(2).mean(-1)[0]


def pool(x):
    return F.avg_pool2d(x, kernel_size=2, padding=[s % 2 for s in x.shape[2:]])


def scale_sizes(h, w):
    """picture sizes of scales 0..4"""
    sizes = [(h, w)]
    for _ in range(len(WEIGHTS) - 1):
        h, w = ((s + 2 * (s % 2) - 2) // 2 + 1 for s in sizes[-1])
        sizes.append((h, w))
    return sizes


def ms_ssim(x, y, dtype=torch.float64, data_range=255.0, device="cpu"):
    """x, y: (3,H,W) or (1,3,H,W) pictures.  -> (MS-SSIM as a Python float, means [5][3][2] (scale, channel, (cs, ssim)))
    computed in `dtype` on `device`; the 15 powers and products are taken in that dtype as well."""
    x = x.reshape(1, *x.shape[-3:]).to(device=device, dtype=dtype)
    y = y.reshape(1, *y.shape[-3:]).to(device=device, dtype=dtype)
    if min(x.shape[-2:]) <= MIN_SIDE:
        raise ValueError(f"the smaller side must exceed {MIN_SIDE} for {len(WEIGHTS)} scales of an {WIN_SIZE}-tap window")
    win = gauss_window(dtype).to(device)
    means, factors = [], []
    for s in range(len(WEIGHTS)):
        cs, ssim = scale_means(x, y, win, data_range)
        means.append(torch.stack((cs, ssim), dim=1))
        factors.append(torch.relu(ssim if s == len(WEIGHTS) - 1 else cs))
        if s < len(WEIGHTS) - 1:
            x, y = pool(x), pool(y)
    wts = torch.tensor(WEIGHTS, dtype=dtype, device=device)
    per_channel = torch.prod(torch.stack(factors, 0) ** wts.view(-1, 1), dim=0)
    flat = torch.cat((per_channel.mean().view(1), torch.stack(means, 0).flatten())).tolist()      # one copy to the host
    rest = flat[1:]
    C = len(rest) // (2 * len(WEIGHTS))
    return flat[0], [[(rest[(s * C + c) * 2], rest[(s * C + c) * 2 + 1]) for c in range(C)] for s in range(len(WEIGHTS))]


# ---------------------------------------------------------------------------------------------------- PSNR side
def harness_pictures(rec_y, rec_c, org_y, org_c, h, w):
    """the harness's statements (test_pMCTF_flex.py:301-317) on CPU float32 tensors ->
    (rounded cropped luma, chroma, rounded RGB of the reconstruction (1,3,h,w), rounded RGB of the original)"""
    from pMCTF.utils.util import ycbcr2rgb, yuv_420_to_444
    ry = torch.round(rec_y.clamp(0, 255.0))[:, :, :h, :w]
    rc = torch.round(rec_c.clamp(0, 255.0))[:, :, :h // 2, :w // 2]
    rgb_rec = torch.round(ycbcr2rgb(yuv_420_to_444((ry, rc[0:1], rc[1:2]))))
    rgb_org = torch.round(ycbcr2rgb(yuv_420_to_444((org_y, org_c[0:1], org_c[1:2]))))
    return ry, rc, rgb_rec, rgb_org


def integer_sse(rec_y, rec_c, org_y, org_c, h, w):
    """(Y, Cb, Cr, RGB) sums of squared differences in int64, and the two RGB pictures"""
    ry, rc, rgb_rec, rgb_org = harness_pictures(rec_y, rec_c, org_y, org_c, h, w)

    def sse(a, b):
        a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
        assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)), "the pictures hold integers"
        d = a.astype(np.int64) - b.astype(np.int64)
        return int((d * d).sum())
    return (sse(ry, org_y), sse(rc[0], org_c[0]), sse(rc[1], org_c[1]), sse(rgb_rec, rgb_org)), rgb_rec, rgb_org


def quality_case(Hp, Wp, h, w, sigma, seed=0):
    """One test picture pair: original from pmctf_synth.synth_yuv420, reconstruction = original + N(0, sigma) float noise on
    the padded planes (strong noise leaves [0, 255]: the clamp is live), with a block of exact k + 0.5 values written over
    each reconstruction plane (round-half-to-even is live).  CPU float32 tensors:
    rec_y (1,1,Hp,Wp), rec_c (2,1,Hp/2,Wp/2), org_y (1,1,h,w), org_c (2,1,h/2,w/2)."""
    import pmctf_synth
    y, cb, cr = (np.ascontiguousarray(p) for p in pmctf_synth.synth_yuv420(w, h, 1, seed=seed + 7)[0])
    org_y = torch.from_numpy(y.astype(np.float32))[None, None]
    org_c = torch.stack((torch.from_numpy(cb.astype(np.float32)), torch.from_numpy(cr.astype(np.float32))))[:, None]
    g = torch.Generator().manual_seed(1000 * seed + Hp + w)
    rec_y = F.pad(org_y, (0, Wp - w, 0, Hp - h)) + sigma * torch.randn((1, 1, Hp, Wp), generator=g)
    rec_c = F.pad(org_c, (0, (Wp - w) // 2, 0, (Hp - h) // 2)) + sigma * torch.randn((2, 1, Hp // 2, Wp // 2), generator=g)
    halves = torch.arange(-2, 258, dtype=torch.float32) + 0.5          # -1.5 .. 257.5: ties inside and outside the clamp
    for plane, rows, cols in ((rec_y[0, 0], h, w), (rec_c[0, 0], h // 2, w // 2), (rec_c[1, 0], h // 2, w // 2)):
        k = min(cols, 52)
        for r in range(halves.numel() // k):                           # 5 rows of 52 inside the crop
            plane[3 + r, 2:2 + k] = halves[r * k:(r + 1) * k]
        assert 3 + halves.numel() // k <= rows
    return rec_y, rec_c, org_y, org_c
