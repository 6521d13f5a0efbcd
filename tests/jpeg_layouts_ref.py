"""numpy restatement of the decoder of other component layouts (mgnns_amd/csrc/jpeg_parse.hpp: mg_jpeg_parse_layout,
jpeg_layouts.hpp, jpeg_decode.hip's layout kernels) on top of jpeg_ref.py: the marker parser with its reason codes and libjpeg's
colour-model rules, the walk over an MCU's block list of sum h_i v_i blocks, the upsampling forms of libjpeg-turbo's jdsample.c with
fancy upsampling and the colour models, CMYK -> RGB as Pillow computes it.  Shared by test_jpeg_layouts_cpu.py and
test_jpeg_layouts_gpu.py; written independently of the HIP code and without PIL.  test_jpeg_layouts_cpu.py ties it to Pillow's
recorded pixels and to live Pillow."""
import numpy as np

from tests import jpeg_ref as R
from tests.jpeg_ref import (ARITHMETIC, COMPONENTS, DNL, EXTENT, MALFORMED, MISSING_TABLES, NOT_JPEG, OK, PRECISION, SCANS, SEG_COEF_OVERFLOW,  # noqa: F401
                      SEG_INVALID_CODE, SEG_OK, SEG_OUT_OF_DATA, UNSUPPORTED_SOF, ZIGZAG, Refused)

FRACTIONAL_SAMPLING, SAMPLING_RANGE = 17, 18
GRAY, YCC, RGB, CMYK, YCCK = range(5)
ROUTED = ((3, 0xC1), (6, None), (7, None), (8, None), (9, None))      # the baseline parser's refusals that go to the layout parser


def routed(reason, detail):
    return reason in (6, 7, 8, 9) or (reason == 3 and detail == 0xC1)


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
    qt, huff, frame, ri, adobe, jfif = {}, {}, None, 0, None, False
    pos = 2
    while True:
        need(pos, 2)
        if d[pos] != 0xFF:
            raise Refused(MALFORMED, pos)
        while pos + 1 < n and d[pos + 1] == 0xFF:
            pos += 1
        need(pos, 2)
        m = d[pos + 1]
        pos += 2
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Refused(MALFORMED, pos)
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
                code = 0
                for l in range(1, 17):
                    code += bits[l - 1]
                    if code > (1 << l):
                        raise Refused(MALFORMED, p)
                    code <<= 1
                huff[(tc, th)] = (bits, list(d[p + 17:p + 17 + cnt]))
                p += 17 + cnt
        elif m == 0xDD:
            if ln != 4:
                raise Refused(MALFORMED, pos)
            ri = u16(body)
        elif m == 0xCC or 0xC9 <= m <= 0xCF:
            raise Refused(ARITHMETIC, m)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8):
            raise Refused(UNSUPPORTED_SOF, m)
        elif m in (0xC0, 0xC1):
            if frame is not None or ln < 8:
                raise Refused(MALFORMED, pos)
            prec, hh, ww, nf = d[body], u16(body + 1), u16(body + 3), d[body + 5]
            if prec != 8:
                raise Refused(PRECISION, prec)
            if ln != 8 + 3 * nf:
                raise Refused(MALFORMED, pos)
            if nf not in (1, 3, 4):
                raise Refused(COMPONENTS, nf)
            if hh == 0:
                raise Refused(DNL)
            if not (1 <= ww <= max_extent and 1 <= hh <= max_extent):
                raise Refused(EXTENT, ww if ww > max_extent else hh)
            comps = [[d[body + 6 + 3 * i], d[body + 7 + 3 * i] >> 4, d[body + 7 + 3 * i] & 15, d[body + 8 + 3 * i]] for i in range(nf)]
            if any(c[3] > 3 for c in comps):
                raise Refused(MALFORMED, pos)
            for c in comps:
                if not (1 <= c[1] <= 4 and 1 <= c[2] <= 4):
                    raise Refused(SAMPLING_RANGE, c[1] * 16 + c[2])
            if nf == 1:
                comps[0][1] = comps[0][2] = 1
            hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
            for c in comps:
                if hmax % c[1] or vmax % c[2]:
                    raise Refused(FRACTIONAL_SAMPLING, c[1] * 16 + c[2])
            if sum(c[1] * c[2] for c in comps) > 10:
                raise Refused(SAMPLING_RANGE, sum(c[1] * c[2] for c in comps))
            frame = (ww, hh, comps, m)
        elif m == 0xDC:
            raise Refused(DNL)
        elif m == 0xE0 and ln >= 16 and bytes(d[body:body + 5]) == b"JFIF\0":
            jfif = True
        elif m == 0xEE and ln >= 14 and bytes(d[body:body + 5]) == b"Adobe":
            adobe = d[body + 11]
        elif m == 0xDA:
            if frame is None:
                raise Refused(MALFORMED, pos)
            ww, hh, comps, sof = frame
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
                if td[-1] > 3 or ta[-1] > 3:
                    raise Refused(MALFORMED, pos)
            if d[body + 1 + 2 * ns] != 0 or d[body + 2 + 2 * ns] != 63 or d[body + 3 + 2 * ns] != 0:
                raise Refused(MALFORMED, pos)
            for i in range(ns):
                if comps[i][3] not in qt or (0, td[i]) not in huff or (1, ta[i]) not in huff:
                    raise Refused(MISSING_TABLES, i)
            pos = end
            break
        pos = end
    ww, hh, comps, sof = frame
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
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
    mcux, mcuy = -(-ww // (8 * hmax)), -(-hh // (8 * vmax))
    nmcu = mcux * mcuy
    nseg = -(-nmcu // ri) if ri else 1
    starts = [begin] + [r + 2 for r in rst]
    ends = rst + [ecs_end]
    segs = [(starts[j], ends[j]) if j < len(starts) else (ecs_end, ecs_end) for j in range(nseg)]
    ids = [c[0] for c in comps]
    if len(comps) == 1:
        colour = GRAY
    elif len(comps) == 3:
        colour = YCC if jfif else ((RGB if adobe == 0 else YCC) if adobe is not None else (RGB if ids == [82, 71, 66] else YCC))
    else:
        colour = YCCK if adobe is not None and adobe != 0 else CMYK
    return dict(width=ww, height=hh, ncomp=len(comps), hmax=hmax, vmax=vmax, h=[c[1] for c in comps], v=[c[2] for c in comps],
                tq=[c[3] for c in comps], td=td, ta=ta, ri=ri, ecs_begin=begin, ecs_end=ecs_end, restarts_found=len(rst), segments=segs,
                qt=qt, huff=huff, mcux=mcux, mcuy=mcuy, colour=colour, sof=sof, mcu_blocks=sum(c[1] * c[2] for c in comps))


def parse(data, max_extent=8192):
    """The layout parser alone -> dict with 'reason' and, when OK, the header fields, tables and segment byte ranges."""
    try:
        out = _parse(bytes(data), max_extent)
        out["reason"], out["layout"] = OK, True
        return out
    except Refused as e:
        return dict(reason=e.reason, detail=e.detail)


def parse_routed(data, max_extent=8192, layouts=True):
    """images.parse_jpeg(..., layouts=): the baseline parser first; the layout parser after its refusals 3 (0xC1), 6, 7, 8, 9."""
    p = R.parse(data, max_extent)
    if layouts and p["reason"] != OK and routed(p["reason"], p.get("detail", 0)):
        p = parse(data, max_extent)
    return p


def entropy_decode(data, p):
    """-> (coefficients per component as int16 [blocks_y, blocks_x, 64] at MCU-padded block counts, status per segment)"""
    nc = p["ncomp"]
    samp = list(zip(p["h"], p["v"]))
    coef = [np.zeros((p["mcuy"] * v, p["mcux"] * h, 64), np.int16) for h, v in samp]
    dc = [R._codes(*p["huff"][(0, t)]) for t in p["td"]]
    ac = [R._codes(*p["huff"][(1, t)]) for t in p["ta"]]
    nmcu = p["mcux"] * p["mcuy"]
    per = p["ri"] if p["ri"] else nmcu
    status = []
    for j, (b, e) in enumerate(p["segments"]):
        br, pred, st = R._Bits(data[b:e]), [0] * nc, SEG_OK
        for mcu in range(j * per, min(nmcu, (j + 1) * per)):
            my, mx = divmod(mcu, p["mcux"])
            for c, by, bx in [(c, by, bx) for c, (h, v) in enumerate(samp) for by in range(v) for bx in range(h)]:
                blk = coef[c][my * samp[c][1] + by, mx * samp[c][0] + bx]
                s = R._symbol(br, dc[c])
                if s < 0 or s > 15:
                    st = SEG_INVALID_CODE
                    break
                pred[c] += R._extend(br.get(s), s)
                blk[0] = np.int16(((pred[c] + 32768) & 0xFFFF) - 32768)
                k = 1
                while k < 64:
                    s = R._symbol(br, ac[c])
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
                    blk[ZIGZAG[k]] = R._extend(br.get(s), s)
                    k += 1
                if st:
                    break
            if st:
                break
        status.append(SEG_OUT_OF_DATA if br.starved() else st)
    return coef, status


def upsample_h1v2(p, H):
    """libjpeg-turbo's h1v2_fancy_upsample: a triangle filter down the columns, the first and last real rows repeated"""
    p = p.astype(np.int32)
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    out = np.empty((2 * p.shape[0], p.shape[1]), np.int32)
    out[0::2] = (3 * p + up + 1) >> 2
    out[1::2] = (3 * p + down + 2) >> 2
    return out[:H]


def upsample(plane, W, H, hr, vr):
    """one component's real samples [dh, dw] -> [H, W], sampled 1 / hr by 1 / vr of the largest (jdsample.c, fancy upsampling)"""
    dh, dw = plane.shape
    if (hr, vr) == (1, 1):
        return plane[:H, :W].astype(np.int32)
    if (hr, vr) == (2, 1) and dw > 2:
        return R.upsample_h2v1(plane, W)[:H]
    if (hr, vr) == (2, 2) and dw > 2:
        return R.upsample_h2v2(plane, W, H)
    if (hr, vr) == (1, 2):
        return upsample_h1v2(plane, H)[:, :W]
    return np.repeat(np.repeat(plane, vr, 0), hr, 1)[:H, :W].astype(np.int32)


def muldiv255(a, b):
    t = a * b + 128
    return (t + (t >> 8)) >> 8


def to_rgb(s, colour):
    """the upsampled components (int32 [H, W] each) -> [H, W, 3] uint8 as Pillow's convert('RGB') gives it"""
    if colour == GRAY:
        return np.stack([s[0]] * 3, 2).astype(np.uint8)
    if colour == YCC:
        return R.ycc_to_rgb(s[0], s[1], s[2])
    if colour == RGB:
        return np.stack(s[:3], 2).astype(np.uint8)
    ink = np.stack(s[:3], 2).astype(np.int32)
    if colour == YCCK:                                  # jdcolor.c, ycck_cmyk_convert: C, M, Y = 255 - (R, G, B)
        ink = 255 - R.ycc_to_rgb(s[0], s[1], s[2]).astype(np.int32)
    nk = s[3].astype(np.int32)[:, :, None]              # Pillow reads the bytes as inverted ink: K' = 255 - K, nk = 255 - K' = K
    return np.clip(nk - muldiv255(255 - ink, nk), 0, 255).astype(np.uint8)


def pixels_from(coef, p):
    W, H = p["width"], p["height"]
    out = []
    for c in range(p["ncomp"]):
        plane = R.idct_plane(coef[c], p["qt"][p["tq"][c]])
        dw, dh = -(-W * p["h"][c] // p["hmax"]), -(-H * p["v"][c] // p["vmax"])
        out.append(upsample(plane[:dh, :dw], W, H, p["hmax"] // p["h"][c], p["vmax"] // p["v"][c]))
    return to_rgb(out, p["colour"])


def decode(data, max_extent=8192):
    """A file of another layout -> ([H,W,3] uint8, status per segment); raises Refused for a file the layout parser does not accept."""
    p = parse(data, max_extent)
    if p["reason"] != OK:
        raise Refused(p["reason"], p.get("detail", 0))
    coef, status = entropy_decode(bytes(data), p)
    return pixels_from(coef, p), status
