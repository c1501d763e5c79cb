"""The pixel layouts of DESIGN 5n restated in numpy, from the layout table alone; shares no code with the product.

unpack(data, layout, h, w, pitch=None, luma_rows=None): the bytes of one picture (uint8 array) -> the packed planar picture
(Y, Cb, Cr; uint8 at 8 bits, uint16 above).  pack(frame, layout, h, w, pitch=None, luma_rows=None, into=None): the inverse;
`into` is the surface written into (a copy is returned), zeros otherwise.  For v210 there is a second formulation, a scalar
loop per pixel over the word table (unpack_v210_scalar, pack_v210_scalar)."""
import numpy as np

# name: (chroma format, depth, container bytes, family)
TABLE = {
    "nv12": ("420", 8, 1, "semi"), "nv21": ("420", 8, 1, "semi"), "nv16": ("422", 8, 1, "semi"),
    "p010": ("420", 10, 2, "semi"), "p012": ("420", 12, 2, "semi"), "p016": ("420", 16, 2, "semi"),
    "p210": ("422", 10, 2, "semi"), "p212": ("422", 12, 2, "semi"), "p216": ("422", 16, 2, "semi"),
    "yuyv": ("422", 8, 1, "pair"), "uyvy": ("422", 8, 1, "pair"),
    "y210": ("422", 10, 2, "pair"), "y212": ("422", 12, 2, "pair"), "y216": ("422", 16, 2, "pair"),
    "v210": ("422", 10, 4, "v210"),
}
# v210: (word, bit) of the six luma values and the three Cb / Cr of a group
V210_Y = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
V210_CB = ((0, 0), (1, 10), (2, 20))
V210_CR = ((0, 20), (2, 0), (3, 10))


def row_bytes(layout, w):
    fmt, depth, container, family = TABLE[layout]
    if family == "v210":
        return (w + 47) // 48 * 128
    return w * container * (2 if family == "pair" else 1)


def geometry(layout, h, w, pitch=None, luma_rows=None):
    """-> (pitch, luma_rows, chroma rows, frame bytes)"""
    fmt, depth, container, family = TABLE[layout]
    pitch = row_bytes(layout, w) if pitch is None else pitch
    luma_rows = h if luma_rows is None else luma_rows
    hc = h // 2 if fmt == "420" else h
    if family == "semi":
        return pitch, luma_rows, hc, pitch * (luma_rows + hc - 1) + row_bytes(layout, w)
    return pitch, luma_rows, hc, pitch * (h - 1) + row_bytes(layout, w)


def samples(layout, h, w):
    fmt = TABLE[layout][0]
    return h * w + 2 * (w // 2) * (h // 2 if fmt == "420" else h)


def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def _rows(data, first_byte, rows, pitch, nbytes):
    """rows x nbytes view of the bytes of `rows` rows starting at first_byte"""
    idx = first_byte + pitch * np.arange(rows)[:, None] + np.arange(nbytes)[None, :]
    return idx


def _words(b):
    """(rows, 2n) bytes -> (rows, n) little-endian 16-bit words"""
    return b[:, 0::2].astype(np.uint16) | (b[:, 1::2].astype(np.uint16) << 8)


def _bytes_of_words(v):
    out = np.empty((v.shape[0], 2 * v.shape[1]), np.uint8)
    out[:, 0::2], out[:, 1::2] = v & 255, v >> 8
    return out


def unpack(data, layout, h, w, pitch=None, luma_rows=None):
    fmt, depth, container, family = TABLE[layout]
    pitch, luma_rows, hc, need = geometry(layout, h, w, pitch, luma_rows)
    data = np.asarray(data, np.uint8)
    assert data.size >= need
    if family == "v210":
        return unpack_v210(data, h, w, pitch)
    get = lambda first, rows, n: (data[_rows(data, first, rows, pitch, n)] if container == 1 else
                                  _words(data[_rows(data, first, rows, pitch, 2 * n)]) >> (16 - depth))
    if family == "semi":
        y = get(0, h, w)
        c = get(pitch * luma_rows, hc, w)
        first = 1 if layout == "nv21" else 0
        cb, cr = c[:, first::2], c[:, 1 - first::2]
    else:
        t = get(0, h, 2 * w)
        if layout == "uyvy":
            y, cb, cr = t[:, 1::2], t[:, 0::4], t[:, 2::4]
        else:
            y, cb, cr = t[:, 0::2], t[:, 1::4], t[:, 3::4]
    return np.concatenate([p.reshape(-1) for p in (y, cb, cr)]).astype(_dtype(depth))


def pack(frame, layout, h, w, pitch=None, luma_rows=None, into=None):
    fmt, depth, container, family = TABLE[layout]
    pitch, luma_rows, hc, need = geometry(layout, h, w, pitch, luma_rows)
    out = np.zeros(need, np.uint8) if into is None else np.array(into, np.uint8)
    assert out.size >= need
    frame = np.asarray(frame).astype(np.uint32) & ((1 << depth) - 1)
    wc = w // 2
    y = frame[:h * w].reshape(h, w)
    cb = frame[h * w:h * w + hc * wc].reshape(hc, wc)
    cr = frame[h * w + hc * wc:].reshape(hc, wc)
    if family == "v210":
        return pack_v210(y, cb, cr, h, w, pitch, out)

    def put(first, v):
        v = v.astype(np.uint16)
        b = v.astype(np.uint8) if container == 1 else _bytes_of_words(v << (16 - depth))
        out[_rows(out, first, v.shape[0], pitch, b.shape[1])] = b

    if family == "semi":
        put(0, y)
        c = np.empty((hc, w), np.uint32)
        first = 1 if layout == "nv21" else 0
        c[:, first::2], c[:, 1 - first::2] = cb, cr
        put(pitch * luma_rows, c)
    else:
        t = np.empty((h, 2 * w), np.uint32)
        if layout == "uyvy":
            t[:, 1::2], t[:, 0::4], t[:, 2::4] = y, cb, cr
        else:
            t[:, 0::2], t[:, 1::4], t[:, 3::4] = y, cb, cr
        put(0, t)
    return out


# --------------------------------------------------------------------------------------------------------------- v210
def unpack_v210(data, h, w, pitch):
    """vectorised: every row as 32-bit words, the three fields of every word, then the table by strides"""
    groups = (w + 5) // 6
    b = data[_rows(data, 0, h, pitch, 16 * groups)].astype(np.uint32)
    words = b[:, 0::4] | (b[:, 1::4] << 8) | (b[:, 2::4] << 16) | (b[:, 3::4] << 24)      # (h, 4 * groups)
    f = np.stack([(words >> s) & 1023 for s in (0, 10, 20)], axis=2).reshape(h, groups, 4, 3)   # [row, group, word, field]
    pick = lambda table: np.stack([f[:, :, wd, bit // 10] for wd, bit in table], axis=2).reshape(h, -1)
    y, cb, cr = pick(V210_Y)[:, :w], pick(V210_CB)[:, :w // 2], pick(V210_CR)[:, :w // 2]
    return np.concatenate([p.reshape(-1) for p in (y, cb, cr)]).astype(np.uint16)


def pack_v210(y, cb, cr, h, w, pitch, out):
    groups = (w + 5) // 6
    row = (w + 47) // 48 * 128
    words = np.zeros((h, row // 4), np.uint32)
    for table, plane in ((V210_Y, y), (V210_CB, cb), (V210_CR, cr)):
        for k, (wd, bit) in enumerate(table):
            v = plane[:, k::len(table)]                                   # value k of every group that has one
            words[:, wd:4 * v.shape[1]:4] |= (v.astype(np.uint32) & 1023) << bit
    assert groups * 4 <= words.shape[1]
    b = np.stack([(words >> s) & 255 for s in (0, 8, 16, 24)], axis=2).reshape(h, row).astype(np.uint8)
    out[_rows(out, 0, h, pitch, row)] = b
    return out


def unpack_v210_scalar(data, h, w, pitch=None):
    """one pixel at a time from the word table"""
    pitch = row_bytes("v210", w) if pitch is None else pitch
    word = lambda r, g, k: int.from_bytes(bytes(data[r * pitch + 16 * g + 4 * k:r * pitch + 16 * g + 4 * k + 4]), "little")
    y, cb, cr = np.zeros((h, w), np.uint16), np.zeros((h, w // 2), np.uint16), np.zeros((h, w // 2), np.uint16)
    for r in range(h):
        for x in range(w):
            g, i = divmod(x, 6)
            wd, bit = V210_Y[i]
            y[r, x] = (word(r, g, wd) >> bit) & 1023
            if x % 2 == 0:
                wd, bit = V210_CB[i // 2]
                cb[r, x // 2] = (word(r, g, wd) >> bit) & 1023
                wd, bit = V210_CR[i // 2]
                cr[r, x // 2] = (word(r, g, wd) >> bit) & 1023
    return np.concatenate([p.reshape(-1) for p in (y, cb, cr)])


def pack_v210_scalar(frame, h, w):
    """one pixel at a time into a zeroed picture of the default pitch"""
    pitch = row_bytes("v210", w)
    words = [[0] * (pitch // 4) for _ in range(h)]
    frame = [int(v) & 1023 for v in frame]
    wc = w // 2
    for r in range(h):
        for x in range(w):
            g, i = divmod(x, 6)
            wd, bit = V210_Y[i]
            words[r][4 * g + wd] |= frame[r * w + x] << bit
            if x % 2 == 0:
                wd, bit = V210_CB[i // 2]
                words[r][4 * g + wd] |= frame[h * w + r * wc + x // 2] << bit
                wd, bit = V210_CR[i // 2]
                words[r][4 * g + wd] |= frame[h * w + h * wc + r * wc + x // 2] << bit
    return np.frombuffer(b"".join(v.to_bytes(4, "little") for row in words for v in row), np.uint8).copy()
