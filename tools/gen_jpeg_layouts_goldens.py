"""tests/golden/jpeg_layouts.npz: JPEG files of the component layouts the baseline decoder refuses ("Other component
layouts") -- CMYK, YCCK, RGB, 4:4:0, 4:1:1, odd mixtures of sampling factors, SOF1, gray labelled 2x2 -- with the pixels Pillow's own
decoder gives for them (Image.open(...).convert('RGB')), files that stay refused with their reason codes, and corrupt files with
the status words of their segments.  Pillow cannot write most of these layouts but opens them: the files are Pillow's 4:2:2 and
4:2:0 files whose SOF0 width, height and sampling bytes are rewritten so that the MCU count and the blocks per MCU stay what they
were (asserted).  The picture is scrambled, the decode is deterministic, and the partial edge MCUs are real.  Build container
only (needs Pillow); rerunning reproduces the committed file byte for byte with the same Pillow / libjpeg-turbo (their versions
are recorded in the file; the zip members carry a fixed date).

    python tools/gen_jpeg_layouts_goldens.py
"""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def picture(w, h, seed, channels=3):
    """smooth gradients with a little noise: every channel varies (K too), flat enough to keep the files small"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin((x + 2 * y) / 5.0), 255.0 * (x + y) / max(w + h - 2, 1)]
    base = np.stack(ch[:channels], 2)
    return np.clip(base + rs.normal(0.0, 6.0, size=base.shape), 0, 255).astype(np.uint8)


def encode(arr, mode=None, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **opts)
    return buf.getvalue()


def segment(data, marker, after=0):
    """-> (offset of the FF, length field) of the first segment with this marker"""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, pos
        m, ln = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        if m == marker and pos >= after:
            return pos, ln
        if m == 0xDA:
            break
        pos += 2 + ln
    raise KeyError("no marker %02X" % marker)


def frame(data):
    """-> (width, height, [(h, v)])"""
    pos, _ = segment(data, 0xC0)
    nf = data[pos + 9]
    return (data[pos + 7] << 8 | data[pos + 8], data[pos + 5] << 8 | data[pos + 6],
            [(data[pos + 11 + 3 * i] >> 4, data[pos + 11 + 3 * i] & 15) for i in range(nf)])


def mcus(w, h, samp):
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    return -(-w // (8 * hmax)), -(-h // (8 * vmax)), sum(a * b for a, b in samp)


def relabel(data, w, h, samp, check=True):
    """rewrite the width, the height and the sampling bytes of SOF0; the MCU grid and the blocks per MCU stay what they were"""
    d = bytearray(data)
    pos, _ = segment(d, 0xC0)
    w0, h0, samp0 = frame(d)
    assert len(samp) == len(samp0)
    if check:
        assert mcus(w, h, samp) == mcus(w0, h0, samp0), (mcus(w, h, samp), mcus(w0, h0, samp0))
    d[pos + 5:pos + 9] = bytes([h >> 8, h & 255, w >> 8, w & 255])
    for i, (a, b) in enumerate(samp):
        d[pos + 11 + 3 * i] = a << 4 | b
    return bytes(d)


def cut(data, marker):
    pos, ln = segment(data, marker)
    return data[:pos] + data[pos + 2 + ln:]


def set_byte(data, at, value):
    d = bytearray(data)
    d[at] = value
    return bytes(d)


S422, S420 = [(2, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]
S440, S411, S1X4 = [(1, 2), (1, 1), (1, 1)], [(4, 1), (1, 1), (1, 1)], [(1, 4), (1, 1), (1, 1)]


def build():
    """-> ({name: bytes} accepted, in order; {name: (bytes, reason)} refused; {name: bytes} corrupt)"""
    acc, ref, bad = {}, {}, {}
    j422 = lambda w, h, seed, **o: encode(picture(w, h, seed), quality=90, subsampling=1, **o)
    j420 = lambda w, h, seed, **o: encode(picture(w, h, seed), quality=90, subsampling=2, **o)
    # 4:4:0: a 4:2:2 file turned on its side; 4:1:1 and 1x4 from 4:2:0 files
    acc["s440_21x45"] = relabel(j422(48, 24, 1), 21, 45, S440)
    acc["s440_16x32"] = relabel(j422(32, 16, 2), 16, 32, S440)
    acc["s440_rst"] = relabel(j422(48, 24, 3, restart_marker_rows=1), 21, 45, S440)
    acc["s440_opt"] = relabel(j422(32, 16, 4, optimize=True), 13, 27, S440)
    acc["s411_61x13"] = relabel(j420(32, 32, 5), 61, 13, S411)
    acc["s411_33x9"] = relabel(j420(32, 32, 6), 33, 9, S411)
    acc["s1x4_16x64"] = relabel(j420(32, 32, 7), 16, 64, S1X4)
    for w in range(1, 6):                                    # widths 1..5: planes of one, two and three samples a row
        acc["s440_w%d" % w] = relabel(j422(16, 8, 10 + w), w, 13, S440)
        acc["s411_w%d" % w] = relabel(j420(16, 16, 20 + w), w, 7, S411)
    # any component may be the small one
    acc["cb2x1"] = relabel(j422(48, 24, 30), 45, 21, [(1, 1), (2, 1), (1, 1)])
    acc["y2x1_cb1x2_cr2x1"] = relabel(j420(32, 32, 31), 29, 27, [(2, 1), (1, 2), (2, 1)])
    # CMYK from a four-channel array whose K varies; YCCK by the Adobe transform byte; one without the Adobe segment
    for name, (w, h), sub in (("s0", (24, 17), 0), ("s2", (37, 29), 2)):
        c = encode(picture(w, h, 40 + sub, 4), "CMYK", quality=90, subsampling=sub)
        pos, _ = segment(c, 0xEE)
        assert c[pos + 4:pos + 9] == b"Adobe" and c[pos + 15] == 0
        acc["cmyk_" + name] = c
        acc["ycck_" + name] = set_byte(c, pos + 15, 2)
    acc["cmyk_noadobe"] = cut(encode(picture(19, 11, 43, 4), "CMYK", quality=90, subsampling=0), 0xEE)
    # RGB: as Pillow writes it (Adobe transform 0, ids R G B), without the Adobe segment, with ids 1 2 3 and the Adobe segment
    rgb = encode(picture(23, 18, 50), quality=90, keep_rgb=True)
    pos, _ = segment(rgb, 0xC0)
    assert bytes(rgb[pos + 10 + 3 * i] for i in range(3)) == b"RGB"
    acc["rgb_adobe"] = rgb
    acc["rgb_ids"] = cut(rgb, 0xEE)
    r123 = bytearray(rgb)
    sos, _ = segment(rgb, 0xDA)
    for i in range(3):
        r123[pos + 10 + 3 * i] = r123[sos + 5 + 2 * i] = i + 1
    acc["rgb_123"] = bytes(r123)
    # SOF1 by its marker; gray labelled 2x2
    s1 = bytearray(j420(27, 21, 60))
    s1[segment(s1, 0xC0)[0] + 1] = 0xC1
    acc["sof1_s2"] = bytes(s1)
    g = encode(picture(19, 14, 61)[:, :, 0], quality=90)
    acc["gray_2x2"] = set_byte(g, segment(g, 0xC0)[0] + 11, 0x22)

    # still refused
    ref["frac_3x1_2x1_1x1"] = (relabel(j420(32, 32, 70), 24, 8, [(3, 1), (2, 1), (1, 1)], check=False), 17)
    ref["factor_5x1"] = (relabel(j422(32, 16, 71), 32, 16, [(5, 1), (1, 1), (1, 1)], check=False), 18)
    ref["blocks_14"] = (relabel(j420(32, 32, 72), 32, 32, [(4, 3), (1, 1), (1, 1)], check=False), 18)
    two = bytearray(j422(16, 8, 73))
    pos, ln = segment(two, 0xC0)
    two[pos + 2:pos + 2 + ln] = bytes([0, 14]) + bytes(two[pos + 4:pos + 9]) + bytes([2]) + bytes(two[pos + 10:pos + 16])
    ref["two_components"] = (bytes(two), 6)
    ref["cmyk_progressive"] = (encode(picture(24, 17, 74, 4), "CMYK", quality=90, progressive=True), 3)
    one = acc["s440_16x32"]
    sos, ln = segment(one, 0xDA)
    eoi = one.rindex(b"\xff\xd9")
    ref["two_scans"] = (one[:eoi] + one[sos:sos + 2 + ln] + b"\x00" + one[eoi:], 10)

    # corrupt: one truncated in its scan, one with sixteen one bits where a code should be
    one = acc["s440_21x45"]
    sos, ln = segment(one, 0xDA)
    bad["s440_truncated"] = one[:sos + 2 + ln + (len(one) - sos - ln) // 2]
    one = acc["cmyk_s2"]
    sos, ln = segment(one, 0xDA)
    at = sos + 2 + ln + 40
    bad["cmyk_bad_code"] = one[:at] + b"\xff\x00\xff\x00\xff\x00" + one[at + 6:]
    return acc, ref, bad


def main():
    import PIL
    from PIL import Image, features
    from tests import jpeg_layouts_ref as L
    from tests import jpeg_ref as R
    acc, ref, bad = build()
    out = {}
    for name, data in acc.items():
        assert R.parse(data)["reason"] in (3, 6, 7, 8, 9), name                 # the baseline parser refuses every one of them
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["pix_" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        got, status = L.decode(data)
        assert not any(status) and np.array_equal(got, out["pix_" + name]), name
    for name, (data, reason) in ref.items():
        assert L.parse_routed(data)["reason"] == reason, (name, L.parse_routed(data))
        out["file_" + name] = np.frombuffer(data, np.uint8)
    statuses = []
    for name, data in bad.items():
        statuses.append(max(L.decode(data)[1]))
        out["file_" + name] = np.frombuffer(data, np.uint8)
    assert statuses == [1, 2], statuses
    try:                                                     # libjpeg itself fails on a fractional factor
        Image.open(io.BytesIO(ref["frac_3x1_2x1_1x1"][0])).convert("RGB")
        raise AssertionError("Pillow opens the fractional file")
    except OSError:
        pass
    out["accepted"] = np.asarray(list(acc))
    out["refused"] = np.asarray(list(ref))
    out["refused_reason"] = np.asarray([r for _, r in ref.values()], np.int32)
    out["corrupt"] = np.asarray(list(bad))
    out["corrupt_status"] = np.asarray(statuses, np.int32)
    out["versions"] = np.asarray(["Pillow " + PIL.__version__, "libjpeg-turbo " + str(features.version("libjpeg_turbo"))])

    path = os.path.join(ROOT, "tests", "golden", "jpeg_layouts.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # (np.savez stamps the members with the current time)
        for key in sorted(out):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            z.writestr(info, buf.getvalue())
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 100 * 1024
    for name in list(acc) + list(ref) + list(bad):
        print("  %-20s %6d bytes" % (name, out["file_" + name].size))


if __name__ == "__main__":
    main()
