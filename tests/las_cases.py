"""Small LAS files built field by field with struct from the ASPRS tables (tests/las_restatement.py quotes them), with the array each
must read as, worked out in plain Python floats: x = X * scale + offset is a multiply and then an add, as numpy's.  Nothing of the
package is imported."""
import struct

import numpy as np

BASE = {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
TYPE_FMT = {1: "<B", 2: "<b", 3: "<H", 4: "<h", 5: "<I", 6: "<i", 7: "<Q", 8: "<q", 9: "<f", 10: "<d"}
I32_MAX = 2 ** 31 - 1


def descriptor(name, dtype, options=0):
    d = struct.pack("<2sBB32s4s24s24s24s24s24s32s", b"", dtype, options, name.encode(), b"", b"", b"", b"", b"", b"", b"a test dimension")
    assert len(d) == 192
    return d


def vlr(user, record_id, body, description=b""):
    v = struct.pack("<H16sHH32s", 0, user.encode(), record_id, len(body), description) + body
    assert len(v) == 54 + len(body)
    return v


def record(fmt, X, Y, Z, class_byte=0, extras=(), pad=0):
    """One point record: the base block of the format with X Y Z, intensity 77, the classification byte where the format keeps it, a
    recognisable filler everywhere else (so a reader that looks at the wrong byte is caught), then the extra values."""
    r = bytearray([0xA5] * BASE[fmt])
    r[0:12] = struct.pack("<3i", X, Y, Z)
    r[12:14] = struct.pack("<H", 77)
    r[15 if fmt <= 5 else 16] = class_byte
    for dtype, v in extras:
        r += struct.pack(TYPE_FMT[dtype], v)
    return bytes(r) + b"\x5A" * pad


def las_file(version, fmt, recs, scale, offset, vlrs=(), legacy_count=None, fmt_byte=None, box=(0.0,) * 6, count=None, record_length=None,
             evlr=b""):
    """Header + VLRs + records (+ trailing bytes, an EVLR for instance)."""
    n = len(recs) if count is None else count
    rl = (len(recs[0]) if recs else BASE[fmt]) if record_length is None else record_length
    hs = {0: 227, 1: 227, 2: 227, 3: 235, 4: 375}[version[1]]
    body = b"".join(vlrs)
    legacy = n if legacy_count is None else legacy_count
    h = struct.pack("<4sHH16sBB32s32sHHHIIBHI5I3d3d6d", b"LASF", 0, 0, b"", version[0], version[1], b"a system", b"a program", 1, 2020, hs,
                    hs + len(body), len(vlrs), fmt if fmt_byte is None else fmt_byte, rl, legacy, legacy, 0, 0, 0, 0, *scale, *offset, *box)
    assert len(h) == 227
    if hs >= 235:
        h += struct.pack("<Q", 0)                                       # waveform data start
    if hs >= 375:
        h += struct.pack("<QIQ15Q", hs + len(body) + n * rl if evlr else 0, 1 if evlr else 0, n, n, *([0] * 14))
    assert len(h) == hs
    return h + body + b"".join(recs) + evlr


def extra_vlr(*dims):
    return vlr("LASF_Spec", 4, b"".join(descriptor(n, t, o) for n, t, o in dims))


def xyz(rows, scale, offset):
    """[[x, y, z], ...] of integer rows in Python floats: one multiply, one add."""
    return [[float(r[a]) * scale[a] + offset[a] for a in range(3)] for r in rows]


S3 = (0.001, 0.001, 0.001)
O0 = (0.0, 0.0, 0.0)

# ---- the writer's own layout, three points, the bytes by hand: X Y Z | intensity | returns class | angle user source | GPS | R G B | treeID
HAND_COORDS = np.array([[1.0, -2.0, 0.25], [0.0, 0.5, 12.345], [-0.001, 3.0, -7.0]])
HAND_LABELS = np.array([0, 7, -1], np.int64)
HAND_RECORDS = bytes.fromhex(
    "e8030000" "30f8ffff" "fa000000" "0000" "09" "02" "00" "00" "0000" "0000000000000000" "000000000000" "00000000"        # 1000 -2000 250, label 0
    "00000000" "f4010000" "39300000" "0000" "09" "04" "00" "00" "0000" "0000000000000000" "7f7f3434b8b8" "07000000"        # 0 500 12345, label 7
    "ffffffff" "b80b0000" "a8e4ffff" "0000" "09" "04" "00" "00" "0000" "0000000000000000" "2f2f06060404" "ffffffff")       # -1 3000 -7000, label -1
HAND_EXTREMES = [-1, -2000, -7000, 1000, 3000, 12345]
HAND_INTS = [(1000, -2000, 250), (0, 500, 12345), (-1, 3000, -7000)]
HAND_READ = np.array([p + [lab] for p, lab in zip(xyz(HAND_INTS, S3, O0), [0.0, 7.0, 4294967295.0])])       # label -1 wraps, as astype(uint32)


def hand_file():
    """The hand records under a header built here (LAS 1.2, format 3, u32 treeID: header 227, one VLR of 54 + 192, data at 473)."""
    recs = [HAND_RECORDS[i * 38:(i + 1) * 38] for i in range(3)]
    f = las_file((1, 2), 3, recs, S3, O0, [extra_vlr(("treeID", 5, 0))])
    assert len(f) == 473 + 3 * 38 and struct.unpack_from("<I", f, 96)[0] == 473 and struct.unpack_from("<H", f, 105)[0] == 38
    return f


def good_cases():
    """name -> (file bytes, the array it reads as, dict of header expectations)."""
    c = {}
    c["hand_1.2_fmt3_u32"] = (hand_file(), HAND_READ, dict(version=(1, 2), point_format=3, record_length=38, count=3,
                                                         extra_dims=[("treeID", 5, 34)]))
    rows = [(1, 2, 3), (-4, 5, -6)]
    c["1.2_fmt0_plain"] = (las_file((1, 2), 0, [record(0, *r) for r in rows], S3, O0), np.array(xyz(rows, S3, O0)),
                           dict(version=(1, 2), point_format=0, record_length=20, count=2, extra_dims=[]))
    # format 1 + u8 treeID; the four combinations of the label rule: (treeID, class) -> label
    combos = [(9, 4, 9.0), (9, 2, 0.0), (0, 1, 0.0), (0, 5, -1.0), (200, 0, 200.0)]
    rows = [(10 * i, -i, i * i) for i in range(len(combos))]
    c["1.2_fmt1_u8_rule"] = (las_file((1, 2), 1, [record(1, *r, class_byte=cl, extras=[(1, t)]) for r, (t, cl, _) in zip(rows, combos)],
                                      S3, O0, [extra_vlr(("treeID", 1, 0))]),
                             np.array([p + [lab] for p, (_, _, lab) in zip(xyz(rows, S3, O0), combos)]),
                             dict(version=(1, 2), point_format=1, record_length=29, count=5, extra_dims=[("treeID", 1, 28)]))
    # 1.4 / format 6, legacy count 0, f64 treeID, per-axis scales, UTM-sized offsets, extreme X; an EVLR after the points is skipped
    sc, of = (0.001, 0.01, 1e-4), (512345.678, 5412345.25, 312.5)
    rows = [(I32_MAX, -I32_MAX, 0), (-I32_MAX, I32_MAX, 1), (-1, 1, -12345), (123456789, -987654321, 55)]
    tids = [3.0, 0.0, 2.5, 0.0]
    cls = [34, 34, 2, 1]                                                  # class 34 is a whole byte in formats 6+: not 1 or 2
    labs = [3.0, -1.0, 0.0, 0.0]
    c["1.4_fmt6_f64_legacy0"] = (las_file((1, 4), 6, [record(6, *r, class_byte=k, extras=[(10, t)]) for r, k, t in zip(rows, cls, tids)],
                                          sc, of, [extra_vlr(("treeID", 10, 0))], legacy_count=0,
                                          evlr=struct.pack("<H16sHQ32s", 0, b"someone", 9, 4, b"") + b"abcd"),
                                 np.array([p + [lab] for p, lab in zip(xyz(rows, sc, of), labs)]),
                                 dict(version=(1, 4), point_format=6, record_length=38, count=4, extra_dims=[("treeID", 10, 30)], scale=sc, offset=of))
    # 1.4 / format 7, two extra dimensions, treeID second (i16, negative ids stay negative), an undocumented 3-byte block before them
    rows = [(5, 6, 7), (8, 9, 10), (11, 12, 13)]
    ex = [(0.5, -3), (1.5, 0), (2.5, 12)]
    cls = [0, 0, 1]
    labs = [-3.0, -1.0, 0.0]
    recs = [record(7, *r, class_byte=k)[:36] + b"\xEE\xEE\xEE" + struct.pack("<f", a) + struct.pack("<h", t) for r, k, (a, t) in zip(rows, cls, ex)]
    c["1.4_fmt7_two_extras"] = (las_file((1, 4), 7, recs, S3, O0, [vlr("someone", 7, b"xyz"), extra_vlr(("blob", 0, 3), ("amplitude", 9, 0), ("treeID", 4, 0))]),
                                np.array([p + [lab] for p, lab in zip(xyz(rows, S3, O0), labs)]),
                                dict(version=(1, 4), point_format=7, record_length=45, count=3,
                                     extra_dims=[("blob", 0, 36), ("amplitude", 9, 39), ("treeID", 4, 43)]))
    # format 2, the class byte carries flag bits: 0b10100010 -> class 2 -> label 0; 0b11100100 -> class 4
    rows = [(1, 1, 1), (2, 2, 2)]
    c["1.2_fmt2_flag_bits"] = (las_file((1, 2), 2, [record(2, *rows[0], class_byte=0b10100010, extras=[(5, 8)]),
                                                    record(2, *rows[1], class_byte=0b11100100, extras=[(5, 8)])], S3, O0, [extra_vlr(("treeID", 5, 0))]),
                               np.array([xyz(rows, S3, O0)[0] + [0.0], xyz(rows, S3, O0)[1] + [8.0]]),
                               dict(version=(1, 2), point_format=2, record_length=30, count=2, extra_dims=[("treeID", 5, 26)]))
    # 1.3 / format 4 (waveform fields ignored), trailing bytes in the record beyond the documented extras, no points at all in another
    rows = [(7, 8, 9)]
    c["1.3_fmt4_padded"] = (las_file((1, 3), 4, [record(4, *rows[0], pad=5)], S3, (1.0, 2.0, 3.0)), np.array(xyz(rows, S3, (1.0, 2.0, 3.0))),
                            dict(version=(1, 3), point_format=4, record_length=62, count=1, extra_dims=[], header_size=235))
    c["1.2_fmt3_empty"] = (las_file((1, 2), 3, [], S3, O0, [extra_vlr(("treeID", 5, 0))], record_length=38), np.zeros((0, 4)),
                           dict(version=(1, 2), point_format=3, record_length=38, count=0))
    return c


def bad_cases():
    """name -> (file bytes, a word the ValueError's message must hold)."""
    good = las_file((1, 2), 0, [record(0, 1, 2, 3), record(0, 4, 5, 6)], S3, O0)
    b = {}
    b["no_signature"] = (b"LASX" + good[4:], "signature")
    b["short_header"] = (good[:100], "header")
    b["header_size_past_end"] = (las_file((1, 4), 6, [], S3, O0)[:300], "header")
    b["short_data"] = (good[:-1], "point data")
    b["record_below_base"] = (las_file((1, 2), 3, [record(0, 1, 2, 3)], S3, O0), "record length")
    patch = lambda f, at, fmt, v: f[:at] + struct.pack(fmt, v) + f[at + struct.calcsize(fmt):]            # noqa: E731
    with_vlr = las_file((1, 2), 0, [record(0, 1, 2, 3)], S3, O0, [vlr("someone", 7, b"x" * 100)])
    b["offset_inside_header"] = (patch(good, 96, "<I", 100), "offset to the point data")
    b["offset_inside_vlrs"] = (patch(with_vlr, 96, "<I", 227 + 60), "offset to the point data")
    b["vlr_count_lies"] = (patch(good, 100, "<I", 4000000000), "offset to the point data")
    b["unknown_format"] = (las_file((1, 4), 6, [record(6, 1, 2, 3)], S3, O0, fmt_byte=11), "point format")
    return b


def compressed_cases():
    """name -> (file bytes, file name): recognised as compressed, never decoded."""
    plain = las_file((1, 2), 0, [record(0, 1, 2, 3)], S3, O0)
    return {"format_bit_7": (las_file((1, 2), 0, [record(0, 1, 2, 3)], S3, O0, fmt_byte=0x80), "a.las"),
            "laszip_vlr": (las_file((1, 2), 0, [record(0, 1, 2, 3)], S3, O0, [vlr("laszip encoded", 22204, b"\0" * 34)]), "b.las"),
            "laz_name": (plain, "c.laz")}
