"""numpy restatement of the baseline JPEG decoder (mgnns_amd/csrc/jpeg_parse.hpp, jpeg_entropy.hpp, jpeg_pixels.hpp,
jpeg_decode.hip): marker parser with its reason codes, Huffman decoding with restart segments and status words, libjpeg's
jidctint 8x8 ("islow"), the "fancy" h2v1 / h2v2 chroma upsampling and the YCbCr -> RGB conversion.  Shared by
test_jpeg_decode_cpu.py and test_jpeg_decode_gpu.py; written independently of the HIP code (bit strings and dictionaries, no
look-ahead tables) and without PIL.  test_jpeg_decode_cpu.py ties it to Pillow's recorded pixels and to live Pillow."""
import numpy as np

# reason codes of the parser (csrc/jpeg_parse.hpp)
OK, NOT_JPEG, MALFORMED, UNSUPPORTED_SOF, ARITHMETIC, PRECISION, COMPONENTS, ADOBE_TRANSFORM, RGB_IDS, SAMPLING, SCANS, DNL, EXTENT, \
    MISSING_TABLES = range(14)
# status words of a segment
SEG_OK, SEG_OUT_OF_DATA, SEG_INVALID_CODE, SEG_COEF_OVERFLOW = range(4)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])            # natural index of the k-th coefficient of the zigzag sequence


class Refused(Exception):
    def __init__(self, reason, detail=0):
        Exception.__init__(self, "reason %d (detail %d)" % (reason, detail))
        self.reason, self.detail = reason, detail


def _parse(d, max_extent):
    n = len(d)

    def need(pos, k):
        if pos + k > n:
            raise Refused(MALFORMED, pos)

    def u16(pos):
        need(pos, 2)
        return d[pos] << 8 | d[pos + 1]

    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused(NOT_JPEG)
    qt, huff, frame, ri, adobe = {}, {}, None, 0, None
    pos = 2
    while True:
        need(pos, 2)
        if d[pos] != 0xFF:
            raise Refused(MALFORMED, pos)
        while pos + 1 < n and d[pos + 1] == 0xFF:          # fill bytes
            pos += 1
        need(pos, 2)
        m = d[pos + 1]
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:    # stand-alone markers
            continue
        if m == 0xD9:
            raise Refused(MALFORMED, pos)                  # EOI before any scan
        ln = u16(pos)
        if ln < 2:
            raise Refused(MALFORMED, pos)
        need(pos, ln)
        body, end = pos + 2, pos + ln
        if m == 0xDB:
            p = body
            while p < end:
                pq, tq = d[p] >> 4, d[p] & 15
                if pq != 0:
                    raise Refused(PRECISION, 16)
                if tq > 3 or p + 65 > end:
                    raise Refused(MALFORMED, p)
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(bytes(d[p + 1:p + 65]), np.uint8)
                qt[tq] = t
                p += 65
        elif m == 0xC4:
            p = body
            while p < end:
                if p + 17 > end:
                    raise Refused(MALFORMED, p)
                tc, th = d[p] >> 4, d[p] & 15
                bits = list(d[p + 1:p + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or p + 17 + cnt > end:
                    raise Refused(MALFORMED, p)
                code, ok = 0, True
                for l in range(1, 17):                     # a code space that is over-subscribed is no Huffman table
                    code += bits[l - 1]
                    if code > (1 << l):
                        ok = False
                    code <<= 1
                if not ok:
                    raise Refused(MALFORMED, p)
                huff[(tc, th)] = (bits, list(d[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif m == 0xDD:
            if ln != 4:
                raise Refused(MALFORMED, pos)
            ri = u16(body)
        elif m == 0xCC or 0xC9 <= m <= 0xCF:
            raise Refused(ARITHMETIC, m)
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8):
            raise Refused(UNSUPPORTED_SOF, m)
        elif m == 0xC0:
            if frame is not None or ln < 8:
                raise Refused(MALFORMED, pos)
            prec, hh, ww, nf = d[body], u16(body + 1), u16(body + 3), d[body + 5]
            if prec != 8:
                raise Refused(PRECISION, prec)
            if ln != 8 + 3 * nf:
                raise Refused(MALFORMED, pos)
            if nf != 1 and nf != 3:
                raise Refused(COMPONENTS, nf)
            if hh == 0:
                raise Refused(DNL)
            if not (1 <= ww <= max_extent and 1 <= hh <= max_extent):
                raise Refused(EXTENT)
            comps = [(d[body + 6 + 3 * i], d[body + 7 + 3 * i] >> 4, d[body + 7 + 3 * i] & 15, d[body + 8 + 3 * i]) for i in range(nf)]
            if nf == 3 and [c[0] for c in comps] == [ord("R"), ord("G"), ord("B")]:
                raise Refused(RGB_IDS)
            if any(c[3] > 3 for c in comps):
                raise Refused(MALFORMED, pos)
            if nf == 1:
                if (comps[0][1], comps[0][2]) != (1, 1):
                    raise Refused(SAMPLING)
            elif (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                raise Refused(SAMPLING)
            frame = (ww, hh, comps)
        elif m == 0xDC:
            raise Refused(DNL)
        elif m == 0xEE and ln >= 14 and bytes(d[body:body + 5]) == b"Adobe":
            adobe = d[body + 11]
        elif m == 0xDA:
            if frame is None:
                raise Refused(MALFORMED, pos)
            ww, hh, comps = frame
            ns = d[body] if ln >= 3 else 0
            if ns != len(comps):
                raise Refused(SCANS, ns)
            if ln != 6 + 2 * ns:
                raise Refused(MALFORMED, pos)
            td, ta = [], []
            for i in range(ns):
                if d[body + 1 + 2 * i] != comps[i][0]:
                    raise Refused(MALFORMED, pos)
                td.append(d[body + 2 + 2 * i] >> 4)
                ta.append(d[body + 2 + 2 * i] & 15)
            if max(td + ta) > 3 or d[body + 1 + 2 * ns] != 0 or d[body + 2 + 2 * ns] != 63 or d[body + 3 + 2 * ns] != 0:
                raise Refused(MALFORMED, pos)
            if adobe == 0 and ns == 3:
                raise Refused(ADOBE_TRANSFORM)
            for i in range(ns):
                if comps[i][3] not in qt or (0, td[i]) not in huff or (1, ta[i]) not in huff:
                    raise Refused(MISSING_TABLES, i)
            pos = end
            break
        pos = end
    # the entropy-coded data: up to the first marker that is neither a stuffed FF nor RSTn
    ww, hh, comps = frame
    hs, vs = comps[0][1], comps[0][2]
    begin, i, rst = pos, pos, []
    while True:
        while i < n and d[i] != 0xFF:
            i += 1
        if i + 1 >= n:
            i = n
            break
        b = d[i + 1]
        if b == 0:
            i += 2
        elif b == 0xFF:
            i += 1
        elif 0xD0 <= b <= 0xD7:
            rst.append(i)
            i += 2
        else:
            break
    ecs_end = i
    # what follows: another scan or DNL is refused; anything else (EOI, nothing, rubbish) ends the file
    while i + 1 < n and d[i] == 0xFF:
        b = d[i + 1]
        if b == 0xFF:
            i += 1
            continue
        if b == 0xD9:
            break
        if b == 0xDA:
            raise Refused(SCANS, 2)
        if b == 0xDC:
            raise Refused(DNL)
        if i + 4 > n:
            break
        i += 2 + (d[i + 2] << 8 | d[i + 3])
    mcux, mcuy = -(-ww // (8 * hs)), -(-hh // (8 * vs))
    nmcu = mcux * mcuy
    nseg = -(-nmcu // ri) if ri else 1
    starts = [begin] + [r + 2 for r in rst]
    ends = rst + [ecs_end]
    segs = [(starts[j], ends[j]) if j < len(starts) else (ecs_end, ecs_end) for j in range(nseg)]
    return dict(width=ww, height=hh, ncomp=len(comps), hs=hs, vs=vs, tq=[c[3] for c in comps], td=td, ta=ta, ri=ri, ecs_begin=begin,
                ecs_end=ecs_end, restarts_found=len(rst), segments=segs, qt=qt, huff=huff, mcux=mcux, mcuy=mcuy)


def parse(data, max_extent=8192):
    """-> dict with 'reason' (OK or a reason code) and, when OK, the header fields, tables and segment byte ranges."""
    try:
        out = _parse(bytes(data), max_extent)
        out["reason"] = OK
        return out
    except Refused as e:
        return dict(reason=e.reason, detail=e.detail)


class _Bits:
    def __init__(self, seg):
        out = bytearray()
        i, n = 0, len(seg)
        while i < n:
            b = seg[i]
            if b == 0xFF:
                if i + 1 < n and seg[i + 1] == 0:
                    i += 1
                else:
                    break                                # a marker, or FF as the segment's last byte: the data ends here
            out.append(b)
            i += 1
        self.bits = np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()
        self.pos = 0

    def get(self, k):
        v = 0
        for _ in range(k):
            v = v << 1 | (self.bits[self.pos] if self.pos < len(self.bits) else 0)
            self.pos += 1
        return v

    def starved(self):
        return self.pos > len(self.bits)


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            table[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for l in range(1, 17):
        code = code << 1 | br.get(1)
        s = table.get((l, code))
        if s is not None:
            return s
    return -1


def _extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def entropy_decode(data, p):
    """-> (coefficients per component as int16 [blocks_y, blocks_x, 64] in natural order at MCU-padded block counts, status per segment)"""
    hs, vs, nc = p["hs"], p["vs"], p["ncomp"]
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    coef = [np.zeros((p["mcuy"] * v, p["mcux"] * h, 64), np.int16) for h, v in samp]
    dc = [_codes(*p["huff"][(0, t)]) for t in p["td"]]
    ac = [_codes(*p["huff"][(1, t)]) for t in p["ta"]]
    nmcu = p["mcux"] * p["mcuy"]
    per = p["ri"] if p["ri"] else nmcu
    status = []
    for j, (b, e) in enumerate(p["segments"]):
        br, pred, st = _Bits(data[b:e]), [0] * nc, SEG_OK
        for mcu in range(j * per, min(nmcu, (j + 1) * per)):
            my, mx = divmod(mcu, p["mcux"])
            for c, (h, v) in enumerate(samp):
                for by in range(v):
                    for bx in range(h):
                        blk = coef[c][my * v + by, mx * h + bx]
                        s = _symbol(br, dc[c])
                        if s < 0 or s > 15:
                            st = SEG_INVALID_CODE
                            break
                        pred[c] += _extend(br.get(s), s)
                        blk[0] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                        k = 1
                        while k < 64:
                            s = _symbol(br, ac[c])
                            if s < 0:
                                st = SEG_INVALID_CODE
                                break
                            r, s = s >> 4, s & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                if k > 64:
                                    st = SEG_COEF_OVERFLOW
                                    break
                                continue
                            k += r
                            if k > 63:
                                st = SEG_COEF_OVERFLOW
                                break
                            blk[ZIGZAG[k]] = _extend(br.get(s), s)
                            k += 1
                        if st:
                            break
                    if st:
                        break
                if st:
                    break
            if st:
                break
        status.append(SEG_OUT_OF_DATA if br.starved() else st)
    return coef, status


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(i0, i1, i2, i3, i4, i5, i6, i7, shift):
    z1 = (i2 + i6) * 4433
    tmp2 = z1 - i6 * 15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0 += z1 + z3
    tmp1 += z2 + z4
    tmp2 += z2 + z3
    tmp3 += z1 + z4
    return [_descale(v, shift) for v in (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1,
                                         tmp11 - tmp2, tmp10 - tmp3)]


def idct_plane(coef, q):
    """int16 [by, bx, 64] x the natural-order quantisation table -> uint8 plane [8 by, 8 bx]"""
    by, bx = coef.shape[:2]
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(by, bx, 8, 8)
    ws = np.stack(_idct_1d(*[x[:, :, r, :] for r in range(8)], 11), 2)             # pass 1: columns
    out = np.stack(_idct_1d(*[ws[:, :, :, c] for c in range(8)], 18), 3)           # pass 2: rows
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return out.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample_h2v1(p, W):
    p = p.astype(np.int32)
    dw = p.shape[1]
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * dw), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out[:, :W]


def upsample_h2v2(p, W, H):
    p = p.astype(np.int32)
    dh, dw = p.shape
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * dh, 2 * dw), np.int32)
    for v, other in ((0, up), (1, down)):
        cs = 3 * p + other
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        row = np.empty((dh, 2 * dw), np.int32)
        row[:, 0::2] = (3 * cs + left + 8) >> 4
        row[:, 1::2] = (3 * cs + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[v::2] = row
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], 2), 0, 255).astype(np.uint8)


def pixels_from(coef, p):
    W, H, hs, vs = p["width"], p["height"], p["hs"], p["vs"]
    planes = [idct_plane(c, p["qt"][t]) for c, t in zip(coef, p["tq"])]
    y = planes[0][:H, :W]
    if p["ncomp"] == 1:
        return np.stack([y, y, y], 2)
    dw, dh = -(-W // hs), -(-H // vs)
    ch = [pl[:dh, :dw] for pl in planes[1:]]
    if (hs, vs) == (2, 1):
        ch = [upsample_h2v1(c, W) for c in ch]
    elif (hs, vs) == (2, 2):
        ch = [upsample_h2v2(c, W, H) for c in ch]
    return ycc_to_rgb(y, ch[0], ch[1])


def decode(data, max_extent=8192):
    """-> ([H,W,3] uint8, status per segment); raises Refused for a file the parser does not accept."""
    p = parse(data, max_extent)
    if p["reason"] != OK:
        raise Refused(p["reason"], p.get("detail", 0))
    coef, status = entropy_decode(bytes(data), p)
    return pixels_from(coef, p), status
