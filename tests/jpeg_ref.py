"""numpy restatement of a baseline JPEG decode as libjpeg-turbo's default path does it (the pixels Pillow hands out): marker
parsing and Huffman decoding, dequantisation, the 13-bit "slow integer" IDCT (jidctint.c: columns descaled by 11, then rows
descaled by 18, + 128, clamped), "fancy" triangle upsampling over the component's own downsampled size with the edge sample
replicated (jdsample.c), 16-bit fixed-point YCbCr -> RGB (jdcolor.c).  For files a conforming encoder wrote: everything is
computed in int64 and nothing is checked for overflow.  The oracle of the C entropy pass (header and coefficients) and, through
the fixture, of the device decode."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
HEADER_BYTES = 512


class Parsed:
    """width, height, components, h_samp, v_samp; per component blocks_w, blocks_h, comp_w, comp_h, quant (natural order,
    [64]), coeffs (int16 [blocks_h * blocks_w, 64], natural order); plane_offset, bytes (the C buffer's layout); dri"""


def _huff_lut(counts, vals):
    """16-bit window -> (length, symbol) tables of one DHT table; length 0: no such code"""
    length = np.zeros(65536, np.int64)
    symbol = np.zeros(65536, np.int64)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(counts[n - 1]):
            lo = code << (16 - n)
            length[lo:lo + (1 << (16 - n))] = n
            symbol[lo:lo + (1 << (16 - n))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), symbol.tolist()


def _windows(seg):
    """for every bit position of the (unstuffed) bytes, the next 16 bits (zeros behind the end)"""
    bits = np.unpackbits(np.frombuffer(seg, np.uint8)).astype(np.int64)
    n = bits.size
    bits = np.concatenate([bits, np.zeros(16, np.int64)])
    w = np.zeros(n + 1, np.int64)
    for k in range(16):
        w += bits[k:k + n + 1] << (15 - k)
    return w.tolist()


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    p = Parsed()
    p.dri = 0
    qt, dc, ac = {}, {}, {}
    pos = 2
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        n = (data[pos] << 8) | data[pos + 1]
        s = data[pos + 2:pos + n]
        pos += n
        if m == 0xDB:
            q = 0
            while q < len(s):
                assert s[q] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(s[q + 1:q + 65], np.uint8)
                qt[s[q] & 15] = t
                q += 65
        elif m == 0xC0:
            assert s[0] == 8
            p.height, p.width, p.components = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(p.components)]
        elif m == 0xC4:
            q = 0
            while q < len(s):
                counts = list(s[q + 1:q + 17])
                nv = sum(counts)
                (ac if s[q] >> 4 else dc)[s[q] & 15] = _huff_lut(counts, list(s[q + 17:q + 17 + nv]))
                q += 17 + nv
        elif m == 0xDD:
            p.dri = (s[0] << 8) | s[1]
        elif m == 0xDA:
            assert s[0] == p.components
            tabs = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(p.components)]
            break
        else:
            assert 0xE0 <= m <= 0xFE, hex(m)
    nc = p.components
    p.h_samp, p.v_samp = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    H, V = p.h_samp, p.v_samp
    mx, my = -(-p.width // (8 * H)), -(-p.height // (8 * V))
    samp = [(H, V) if c == 0 else (1, 1) for c in range(nc)]
    p.blocks_w = [mx * h for h, v in samp]
    p.blocks_h = [my * v for h, v in samp]
    p.comp_w = [-(-p.width * h // H) for h, v in samp]
    p.comp_h = [-(-p.height * v // V) for h, v in samp]
    p.quant = [qt[comps[c][3]] for c in range(nc)]
    p.plane_offset, off = [], HEADER_BYTES
    for c in range(nc):
        p.plane_offset.append(off)
        off += p.blocks_w[c] * p.blocks_h[c] * 128
    p.bytes = off
    # the entropy-coded data: segments between restart markers, unstuffed
    segs, cur = [], bytearray()
    while True:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
        elif data[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
        elif 0xD0 <= data[pos + 1] <= 0xD7:
            assert data[pos + 1] == 0xD0 + len(segs) % 8
            segs.append(bytes(cur))
            cur = bytearray()
            pos += 2
        else:
            assert data[pos + 1] == 0xD9
            segs.append(bytes(cur))
            break
    p.coeffs = [np.zeros((p.blocks_w[c] * p.blocks_h[c], 64), np.int16) for c in range(nc)]
    zz = ZIGZAG.tolist()
    mcus = [(j, i) for j in range(my) for i in range(mx)]
    per = p.dri or len(mcus)
    assert len(segs) == -(-len(mcus) // per)
    for si, seg in enumerate(segs):
        w, bit = _windows(seg), 0
        pred = [0] * nc
        for (j, i) in mcus[si * per:(si + 1) * per]:
            for c in range(nc):
                dlen, dsym = dc[tabs[c][0]]
                alen, asym = ac[tabs[c][1]]
                for v in range(samp[c][1]):
                    for h in range(samp[c][0]):
                        blk = p.coeffs[c][(j * samp[c][1] + v) * p.blocks_w[c] + i * samp[c][0] + h]
                        x = w[bit]
                        assert dlen[x]
                        bit += dlen[x]
                        s_ = dsym[x]
                        if s_:
                            pred[c] += _extend(w[bit] >> (16 - s_), s_)
                            bit += s_
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            x = w[bit]
                            assert alen[x]
                            bit += alen[x]
                            r, s_ = asym[x] >> 4, asym[x] & 15
                            if s_ == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            blk[zz[k]] = _extend(w[bit] >> (16 - s_), s_)
                            bit += s_
                            k += 1
        assert bit <= 8 * len(seg)
    return p


def _idct8(i):
    """jidctint.c's 8-point pass on the eight input arrays i[0..7]; the eight outputs before the descale"""
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    z2, z3 = i[0], i[4]
    tmp0 = (z2 + z3) << 13
    tmp1 = (z2 - z3) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def idct_plane(coeffs, quant, blocks_h, blocks_w):
    """uint8 [blocks_h * 8, blocks_w * 8]: the padded plane of one component"""
    x = coeffs.astype(np.int64).reshape(-1, 8, 8) * quant.reshape(1, 8, 8)
    ws = np.stack([(o + (1 << 10)) >> 11 for o in _idct8([x[:, k, :] for k in range(8)])], axis=1)  # columns: over the row index
    out = np.stack([(o + (1 << 17)) >> 18 for o in _idct8([ws[:, :, k] for k in range(8)])], axis=2)
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return out.reshape(blocks_h, blocks_w, 8, 8).transpose(0, 2, 1, 3).reshape(blocks_h * 8, blocks_w * 8)


def _left(a):
    return np.concatenate([a[:, :1], a[:, :-1]], axis=1)


def _right(a):
    return np.concatenate([a[:, 1:], a[:, -1:]], axis=1)


def _interleave(even, odd, axis):
    shape = list(even.shape)
    shape[axis] *= 2
    out = np.empty(shape, np.int64)
    sl = [slice(None)] * 2
    sl[axis] = slice(0, None, 2)
    out[tuple(sl)] = even
    sl[axis] = slice(1, None, 2)
    out[tuple(sl)] = odd
    return out


def upsample(plane, h_samp, v_samp):
    """plane: the component's own downsampled samples [comp_h, comp_w]; int64 [comp_h * v_samp, comp_w * h_samp]"""
    a = plane.astype(np.int64)
    if h_samp == 1 and v_samp == 1:
        return a
    if v_samp == 1:
        return _interleave((3 * a + _left(a) + 1) >> 2, (3 * a + _right(a) + 2) >> 2, 1)
    up = np.concatenate([a[:1], a[:-1]], axis=0)
    down = np.concatenate([a[1:], a[-1:]], axis=0)
    s = _interleave(3 * a + up, 3 * a + down, 0)
    return _interleave((3 * s + _left(s) + 8) >> 4, (3 * s + _right(s) + 7) >> 4, 1)


def pixels(p):
    """uint8 [h, w, 3] (RGB) or [h, w] (grey) of a parse() result"""
    planes = [idct_plane(p.coeffs[c], p.quant[c], p.blocks_h[c], p.blocks_w[c]) for c in range(p.components)]
    h, w = p.height, p.width
    if p.components == 1:
        return planes[0][:h, :w].copy()
    y = planes[0][:h, :w].astype(np.int64)
    cb, cr = (upsample(planes[c][:p.comp_h[c], :p.comp_w[c]], p.h_samp, p.v_samp)[:h, :w] - 128 for c in (1, 2))
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    return pixels(parse(data))
