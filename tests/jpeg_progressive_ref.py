"""numpy restatement of the progressive JPEG decoder (mgnns_amd/csrc/jpeg_parse.hpp mg_jpeg_parse_progressive,
jpeg_progressive.hpp): the marker parser with its scan list, levels, segments, latched quantisation tables and reason codes, and
the four procedures of T.81 Annex G (DC first, DC refinement, AC first, AC refinement) with status words.  Written independently
of the HIP code (bit strings and dictionaries, no look-ahead tables, no masks) and without PIL; the IDCT, the chroma upsampling
and the colour conversion are tests/jpeg_ref.py's (pixels_from below adds the one case it leaves out).  test_jpeg_progressive_cpu.py ties it to Pillow's recorded pixels and to live
Pillow, and the library's parser and decoder body to it."""
import numpy as np

from tests import jpeg_ref as R
from tests.jpeg_ref import (ADOBE_TRANSFORM, ARITHMETIC, COMPONENTS, DNL, EXTENT, MALFORMED, MISSING_TABLES, NOT_JPEG, OK, PRECISION,  # noqa: F401
                            RGB_IDS, SAMPLING, SEG_COEF_OVERFLOW, SEG_INVALID_CODE, SEG_OK, SEG_OUT_OF_DATA, UNSUPPORTED_SOF, ZIGZAG, Refused)

INCOMPLETE_PROGRESSION, ILLEGAL_PROGRESSION, TOO_MANY_SCANS = 14, 15, 16
MAX_SCANS = 32


class _EndOfFile(Exception):
    pass


def _cdiv(a, b):
    return -(-a // b)


def _parse(d, max_extent):
    n = len(d)
    scans = []

    def bad(pos):
        """what cannot be read: malformed before the first scan, the end of the file after it"""
        raise _EndOfFile() if scans else Refused(MALFORMED, pos)

    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused(NOT_JPEG)
    qt, huff, frame, ri, adobe = {}, {}, None, 0, None
    latched, al_of, level_of, dc_level = {}, {}, {}, {}
    pos = 2
    try:
        while True:
            if pos + 2 > n or d[pos] != 0xFF:
                bad(pos)
            while pos + 1 < n and d[pos + 1] == 0xFF:          # fill bytes
                pos += 1
            if pos + 2 > n:
                bad(pos)
            m = d[pos + 1]
            pos += 2
            if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:    # stand-alone markers
                continue
            if m == 0xD9:
                bad(pos)                                       # EOI: before any scan it is malformed
            if pos + 2 > n:
                bad(pos)
            ln = d[pos] << 8 | d[pos + 1]
            if ln < 2 or pos + ln > n:
                bad(pos)
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
                ri = d[body] << 8 | d[body + 1]
            elif m == 0xCC or 0xC9 <= m <= 0xCF:
                raise Refused(ARITHMETIC, m)
            elif m in (0xC0, 0xC1, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8):
                raise Refused(UNSUPPORTED_SOF, m)
            elif m == 0xC2:
                if frame is not None or ln < 8:
                    raise Refused(MALFORMED, pos)
                prec, hh, ww, nf = d[body], d[body + 1] << 8 | d[body + 2], d[body + 3] << 8 | d[body + 4], d[body + 5]
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
                if len(scans) == MAX_SCANS:
                    raise Refused(TOO_MANY_SCANS, MAX_SCANS + 1)
                ww, hh, comps = frame
                ns = d[body] if ln >= 3 else 0
                if ns < 1 or ns > len(comps) or ln != 6 + 2 * ns:
                    raise Refused(MALFORMED, pos)
                ids = [c[0] for c in comps]
                cs, td, ta, c = [], [], [], 0
                for i in range(ns):                            # the frame's components, in the frame's order
                    while c < len(comps) and ids[c] != d[body + 1 + 2 * i]:
                        c += 1
                    if c >= len(comps):
                        raise Refused(MALFORMED, pos)
                    cs.append(c)
                    c += 1
                    td.append(d[body + 2 + 2 * i] >> 4)
                    ta.append(d[body + 2 + 2 * i] & 15)
                if max(td + ta) > 3:
                    raise Refused(MALFORMED, pos)
                ss, se, ah, al = d[body + 1 + 2 * ns], d[body + 2 + 2 * ns], d[body + 3 + 2 * ns] >> 4, d[body + 3 + 2 * ns] & 15
                if adobe == 0 and len(comps) == 3:
                    raise Refused(ADOBE_TRANSFORM)
                # T.81 G.1.1.1.1 and the scans before
                legal = (se == 0) if ss == 0 else (ss <= se <= 63 and ns == 1)
                legal = legal and (ah == 0 or al == ah - 1) and al <= 13
                for c in cs:
                    if ss != 0 and (c, 0) not in al_of:
                        legal = False                          # AC before the component's DC
                    for k in range(ss, min(se, 63) + 1):
                        prev = al_of.get((c, k))
                        if (ah != 0) if prev is None else (ah == 0 or ah != prev):
                            legal = False
                if not legal:
                    raise Refused(ILLEGAL_PROGRESSION, len(scans))
                dc_tables, ac_table, level = {}, None, 0
                for i, c in enumerate(cs):
                    if c not in latched:                       # the quantisation table in force at the component's first scan
                        if comps[c][3] not in qt:
                            raise Refused(MISSING_TABLES, c)
                        latched[c] = qt[comps[c][3]].copy()
                    if ss == 0 and ah == 0:
                        if (0, td[i]) not in huff:
                            raise Refused(MISSING_TABLES, c)
                        dc_tables[c] = huff[(0, td[i])]
                    elif ss != 0:
                        if (1, ta[i]) not in huff:
                            raise Refused(MISSING_TABLES, c)
                        ac_table = huff[(1, ta[i])]
                    touched = [level_of.get((c, k), -1) for k in range(ss, se + 1)] + ([dc_level[c]] if ss != 0 else [])
                    level = max([level] + [t + 1 for t in touched])
                for c in cs:
                    if ss == 0:
                        dc_level.setdefault(c, level)
                    for k in range(ss, se + 1):
                        al_of[(c, k)], level_of[(c, k)] = al, level
                hs, vs = comps[0][1], comps[0][2]
                if ns > 1:
                    units = -(-ww // (8 * hs)) * -(-hh // (8 * vs))
                else:
                    h, v = comps[cs[0]][1], comps[cs[0]][2]
                    units = _cdiv(_cdiv(ww * h, hs), 8) * _cdiv(_cdiv(hh * v, vs), 8)         # not the MCU-padded counts
                # the entropy-coded data: up to the first marker that is neither a stuffed FF nor RSTn
                begin, i, rst = end, end, []
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
                nseg = -(-units // ri) if ri else 1
                starts, ends = [begin] + [r + 2 for r in rst], rst + [i]
                per = ri if ri else units
                segs = [((starts[j], ends[j]) if j < len(starts) else (i, i)) + (j * per, min(per, units - j * per)) for j in range(nseg)]
                scans.append(dict(comps=cs, ss=ss, se=se, ah=ah, al=al, ri=ri, level=level, dc_tables=dc_tables, ac_table=ac_table, units=units,
                                  segments=segs, ecs=(begin, i), restarts=len(rst)))
                pos = i
                continue
            pos = end
    except _EndOfFile:
        pass
    ww, hh, comps = frame
    for c in range(len(comps)):
        for k in range(64):
            if al_of.get((c, k)) != 0:
                raise Refused(INCOMPLETE_PROGRESSION, 64 * c + k)
    hs, vs = comps[0][1], comps[0][2]
    return dict(width=ww, height=hh, ncomp=len(comps), hs=hs, vs=vs, mcux=-(-ww // (8 * hs)), mcuy=-(-hh // (8 * vs)), scans=scans,
                levels=1 + max(s["level"] for s in scans), qt=[latched[c] for c in range(len(comps))], tq=list(range(len(comps))))


def parse(data, max_extent=8192):
    """-> dict with 'reason' (OK or a reason code) and, when OK, the frame, the scans (with their levels, tables and segments) and the
    latched quantisation tables."""
    try:
        out = _parse(bytes(data), max_extent)
        out["reason"] = OK
        return out
    except Refused as e:
        return dict(reason=e.reason, detail=e.detail)


def _correct(blk, pos, br, p1):
    """a correction bit for a coefficient that is already non-zero"""
    if br.get(1) and not (int(blk[pos]) & p1):
        blk[pos] += p1 if blk[pos] >= 0 else -p1


def _decode_segment(br, p, sc, unit0, nunits, coef, stats):
    hs, vs, W, H = p["hs"], p["vs"], p["width"], p["height"]
    ss, se, ah, al, cs = sc["ss"], sc["se"], sc["ah"], sc["al"], sc["comps"]
    samp = [(hs, vs), (1, 1), (1, 1)]
    if len(cs) > 1:                                            # MCUs: every component's h x v blocks
        order = []
        for u in range(unit0, unit0 + nunits):
            my, mx = divmod(u, p["mcux"])
            for c in cs:
                h, v = samp[c]
                order += [(c, my * v + by, mx * h + bx) for by in range(v) for bx in range(h)]
    else:                                                      # the component's own blocks, in raster order
        c = cs[0]
        h, v = samp[c]
        bw = _cdiv(_cdiv(W * h, hs), 8)
        order = [(c,) + divmod(u, bw) for u in range(unit0, unit0 + nunits)]
    p1 = 1 << al
    if ss == 0:
        tables = {c: R._codes(*t) for c, t in sc["dc_tables"].items()}
        pred = {c: 0 for c in cs}
        for c, by, bx in order:
            blk = coef[c][by, bx]
            if ah == 0:
                s = R._symbol(br, tables[c])
                if s < 0 or s > 15:
                    return SEG_INVALID_CODE
                pred[c] += R._extend(br.get(s), s)
                blk[0] = np.int16((((pred[c] << al) + 32768) & 0xFFFF) - 32768)
            elif br.get(1):
                blk[0] |= p1
        return SEG_OK
    table = R._codes(*sc["ac_table"])
    zz = [int(z) for z in ZIGZAG]
    eobrun = 0
    for j, (c, by, bx) in enumerate(order):
        blk = coef[c][by, bx]
        k = ss
        if ah == 0:                                            # ---- AC first (G.1.2.2)
            if eobrun > 0:
                eobrun -= 1
                continue
            while k <= se:
                s = R._symbol(br, table)
                if s < 0:
                    return SEG_INVALID_CODE
                r, s = s >> 4, s & 15
                if s:
                    k += r
                    if k > se:
                        return SEG_COEF_OVERFLOW
                    blk[zz[k]] = R._extend(br.get(s), s) * p1
                    k += 1
                elif r == 15:
                    k += 16
                    if k > se + 1:
                        return SEG_COEF_OVERFLOW
                else:
                    stats["eob_cat_max"] = max(stats.get("eob_cat_max", 0), r)
                    eobrun = (1 << r) + br.get(r) - 1
                    break
            continue
        # ---- AC refinement (G.1.2.3)
        if eobrun == 0:
            while k <= se:
                s = R._symbol(br, table)
                if s < 0:
                    return SEG_INVALID_CODE
                r, s = s >> 4, s & 15
                new = 0
                if s:
                    if s != 1:
                        return SEG_INVALID_CODE
                    new = p1 if br.get(1) else -p1
                elif r != 15:
                    stats["eob_cat_max"] = max(stats.get("eob_cat_max", 0), r)
                    eobrun = (1 << r) + br.get(r)
                    break
                found = False
                while k <= se:                                 # pass non-zero coefficients (a bit each) and r zero ones
                    if blk[zz[k]] != 0:
                        _correct(blk, zz[k], br, p1)
                    else:
                        if r == 0:
                            found = True
                            break
                        r -= 1
                    k += 1
                if not found:
                    return SEG_COEF_OVERFLOW                   # the new coefficient's place, or the 16th zero of a ZRL, lies beyond Se
                if new:
                    blk[zz[k]] = new
                k += 1
        if eobrun > 0:                                         # the rest of the band: correction bits only
            band = blk[[zz[q] for q in range(k, se + 1)]] if k <= se else np.zeros(0)
            if band.any():
                for q in range(k, se + 1):
                    if blk[zz[q]] != 0:
                        _correct(blk, zz[q], br, p1)
            eobrun -= 1
    return SEG_OK


def entropy_decode(data, p):
    """-> (coefficients per component as int16 [blocks_y, blocks_x, 64] in natural order at MCU-padded block counts, [(scan, segment
    of the scan, status)], statistics); the scans run in file order, which every level order refines"""
    samp = [(p["hs"], p["vs"])] + [(1, 1)] * (p["ncomp"] - 1)
    coef = [np.zeros((p["mcuy"] * v, p["mcux"] * h, 64), np.int16) for h, v in samp]
    status, stats = [], {}
    for k, sc in enumerate(p["scans"]):
        for j, (b, e, unit0, nunits) in enumerate(sc["segments"]):
            br = R._Bits(data[b:e])
            st = _decode_segment(br, p, sc, unit0, nunits, coef, stats)
            status.append((k, j, SEG_OUT_OF_DATA if br.starved() else st))
    return coef, status, stats


def pixels_from(coef, p):
    """jpeg_ref's planes, upsampling and colour conversion -- with libjpeg's rule that a chroma plane of at most two samples a row is
    replicated, not filtered (jdsample.c: "fancy" upsampling needs downsampled_width > 2), which jpeg_ref.pixels_from leaves out"""
    W, H, hs, vs = p["width"], p["height"], p["hs"], p["vs"]
    if p["ncomp"] == 1 or hs == 1 or _cdiv(W, hs) > 2:
        return R.pixels_from(coef, p)
    planes = [R.idct_plane(c, q) for c, q in zip(coef, p["qt"])]
    ch = [pl[:_cdiv(H, vs), :_cdiv(W, hs)].repeat(hs, 1).repeat(vs, 0)[:H, :W] for pl in planes[1:]]
    return R.ycc_to_rgb(planes[0][:H, :W], ch[0], ch[1])


def decode(data, max_extent=8192):
    """-> ([H,W,3] uint8, [(scan, segment, status)], statistics); raises Refused for a file the parser does not accept."""
    p = parse(data, max_extent)
    if p["reason"] != OK:
        raise Refused(p["reason"], p.get("detail", 0))
    coef, status, stats = entropy_decode(bytes(data), p)
    return pixels_from(coef, p), status, stats
