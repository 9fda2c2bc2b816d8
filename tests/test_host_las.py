"""Host tests of the LAS reader and writer (treelearn_amd/util/las.py): the numpy restatement against files built by hand,
read_header on every case and every malformed file, the format check of the segment command line, and the C declarations.  No GPU."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import las_cases as cases
import las_restatement as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_of_the_layout():
    assert [struct.calcsize(f) for f in (ref.HEADER, ref.HEADER + "Q", ref.HEADER + "QQIQ15Q", ref.VLR, ref.DESCRIPTOR)] == [227, 235, 375, 54, 192]
    assert [ref.BASE_LENGTH[f] for f in range(11)] == [20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67]


def test_restatement_reads_the_hand_cases():
    for name, (buf, want, _) in cases.good_cases().items():
        got = ref.read(buf)
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, got, want)


def test_restatement_writes_the_hand_bytes():
    rec = ref.records(cases.HAND_COORDS, cases.HAND_LABELS)
    assert rec.tobytes() == cases.HAND_RECORDS
    assert ref.records(cases.HAND_COORDS.astype(np.float32), cases.HAND_LABELS).tobytes() == cases.HAND_RECORDS     # f32 is widened exactly
    assert ref.extremes(rec).tolist() == cases.HAND_EXTREMES
    whole = ref.write(cases.HAND_COORDS, cases.HAND_LABELS, (0.0, 0.0, 0.0), (123, 2024))
    assert len(whole) == 473 + 3 * 38 and whole[473:] == cases.HAND_RECORDS
    h = ref.parse(whole)
    assert (h["version"], h["point_format"], h["record_length"], h["count"], h["offset_to_points"]) == ((1, 2), 3, 38, 3, 473)
    assert h["extra_dims"] == [("treeID", 5, 34)] and struct.unpack_from("<HH", whole, 90) == (123, 2024)
    assert struct.unpack_from("<5I", whole, 111) == (3, 0, 0, 0, 0)
    assert h["mins"] == (-1 * 0.001 + 0.0, -2000 * 0.001 + 0.0, -7000 * 0.001 + 0.0) and h["maxs"] == (1000 * 0.001, 3000 * 0.001, 12345 * 0.001)
    assert np.array_equal(ref.read(whole), cases.HAND_READ)
    assert np.array_equal(ref.read(cases.hand_file()), cases.HAND_READ)           # the same records under the header built field by field


def test_restatement_rounding_and_refusals():
    # quotients exactly on k + 0.5 (scale 0.5 and offset 0 make them exact): half to even, both parities, both signs
    x = np.array([0.25, 0.75, 1.25, -0.25, -0.75, -1.25])
    q, ok = ref.quantise(np.stack([x, x, x], 1), (0.5,) * 3, (0.0,) * 3)
    assert ok.all() and q[:, 0].tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, -2.0]
    for bad in (np.nan, np.inf, -np.inf, 2147483.648, -2147483.649):
        with pytest.raises(ValueError):
            ref.records(np.array([[0.0, bad, 0.0]]), [1])
    ref.records(np.array([[2147483.647, -2147483.648, 0.0]]), [1])             # the extreme integers themselves are written


def test_contraction_would_show():
    """The decode test compares bits, so it has to be able to see a fused multiply-add: it changes a good share of these values."""
    X = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, 2000)
    two = X * np.float64(0.001) + np.float64(512345.678)
    one = ref.fma_read_x(X, 0.001, 512345.678)
    assert 0.1 < np.mean(two != one) < 0.6


def _write(tmp_path, name, buf):
    p = tmp_path / name
    p.write_bytes(buf)
    return str(p)


def test_read_header_on_every_case(tmp_path):
    from treelearn_amd.util.las import read_header
    for name, (buf, want, expect) in cases.good_cases().items():
        h = read_header(_write(tmp_path, name + ".las", buf))
        r = ref.parse(buf)
        assert not h.compressed
        for k in ("version", "point_format", "record_length", "count", "header_size", "offset_to_points", "extra_dims"):
            assert getattr(h, k) == r[k], (name, k, getattr(h, k), r[k])
        for k in ("scale", "offset", "mins", "maxs"):
            assert tuple(getattr(h, k)) == tuple(r[k]), (name, k)
        for k, v in expect.items():
            assert (tuple(getattr(h, k)) if k in ("scale", "offset") else getattr(h, k)) == v, (name, k, getattr(h, k), v)
        assert (h.extra("treeID") is not None) == (want.shape[1] == 4), name


def test_read_header_errors(tmp_path):
    from treelearn_amd.util.las import read_header, read_las
    for name, (buf, word) in cases.bad_cases().items():
        p = _write(tmp_path, name + ".las", buf)
        with pytest.raises(ValueError, match=word):
            ref.parse(buf)
        with pytest.raises(ValueError, match=word) as e:
            read_header(p)
        assert p in str(e.value)
        with pytest.raises(ValueError, match=word):
            read_las(p)                                                          # before any GPU work
    # a treeID descriptor that points past the record
    buf = cases.las_file((1, 2), 0, [cases.record(0, 1, 2, 3)], cases.S3, cases.O0, [cases.extra_vlr(("treeID", 5, 0))])
    with pytest.raises(ValueError, match="outside the 20-byte record"):
        read_header(_write(tmp_path, "lying_extra.las", buf))


def test_compressed_files_are_recognised_not_guessed(tmp_path):
    from treelearn_amd.util.las import read_header, read_las
    try:
        import laspy  # noqa: F401
        have = True
    except ImportError:
        have = False
    for name, (buf, fname) in cases.compressed_cases().items():
        p = _write(tmp_path, fname, buf)
        assert read_header(p).compressed and ref.parse(buf, fname)["compressed"], name
        if not have:
            with pytest.raises(ImportError, match="laspy"):
                read_las(p)


def test_check_formats_las_without_laspy():
    from treelearn_amd.util.segment import check_formats
    check_formats(["las"])                                                       # written natively: no module needed
    check_formats(["npz", "las", "txt"])
    try:
        import laspy  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="laspy"):
            check_formats(["laz"])
    with pytest.raises(ValueError, match="unknown save format"):
        check_formats(["ply"])


def test_segment_cli_accepts_las(tmp_path):
    """--formats las passes the format check; the run then stops at the weights file, before any output directory exists."""
    forest = tmp_path / "plot.npy"
    np.save(forest, np.zeros((10, 3)))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "treelearn_amd.util.segment", "--forest", str(forest), "--weights", str(tmp_path / "missing.pth"),
                        "--out", str(out), "--formats", "las"], capture_output=True, text=True, timeout=120, cwd=REPO,
                       env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 2 and "--weights" in p.stderr and "no such file" in p.stderr, p.stderr[-400:]
    assert "laspy" not in p.stderr and not out.exists()


def test_load_forest_dispatch_and_untouched_loaders(tmp_path):
    from treelearn_amd.util import eval as ev
    from treelearn_amd.util.segment import load_forest
    with pytest.raises(ValueError, match="expected .npy, .npz or .txt"):
        ev.load_points(str(tmp_path / "x.las"))                                 # load_points keeps its behaviour
    with pytest.raises(ValueError, match="signature"):
        load_forest(_write(tmp_path, "bad.las", b"nope" * 100))                  # .las goes to the LAS reader
    np.save(tmp_path / "a.npy", np.arange(12.0).reshape(4, 3))
    assert load_forest(str(tmp_path / "a.npy")).shape == (4, 3)
    with pytest.raises(ValueError, match="signature"):
        ev._load_labelled(_write(tmp_path, "bad2.LAS", b"nope" * 100))


def test_writer_header_matches_restatement():
    from treelearn_amd.util import las
    for count, off, ext in ((3, (0.0, 0.0, 0.0), cases.HAND_EXTREMES), (0, (0.0, 0.0, 0.0), [0] * 6),
                            (5, (512345.678, 5412345.25, 312.5), [-2 ** 31, -5, 0, 2 ** 31 - 1, 7, 123456])):
        assert las.header_bytes(count, off, ext, (200, 2031)) == ref.header(count, off, ext, (200, 2031)), count
    assert len(las.header_bytes(1, (0, 0, 0), [0] * 6)) == 473                   # created defaults to today
    with pytest.raises(ValueError, match="32-bit point count"):
        las.header_bytes(1 << 32, (0, 0, 0), [0] * 6)
    assert las.BASE_LENGTH == tuple(ref.BASE_LENGTH[f] for f in range(11)) and las.RECORD_LENGTH == 38


def test_new_entries_declared_and_bound():
    """include/treelearn_hip.h and _hip.PROTOTYPES agree on the two entries: names, and the number and kinds of the arguments."""
    import ctypes
    from treelearn_amd import _hip
    hdr = open(os.path.join(REPO, "include", "treelearn_hip.h")).read()
    for name in ("tl_las_decode", "tl_las_encode"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m, f"{name} is not declared"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _hip.PROTOTYPES[name]
        assert res is ctypes.c_int32 and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            if "[3]" in p:
                want = ctypes.c_double * 3
            elif "*" in p or p.startswith("tl_stream_t"):
                want = ctypes.c_void_p
            elif p.startswith("int64_t"):
                want = ctypes.c_int64
            else:
                assert p.startswith(("int32_t", "int ")), p
                want = ctypes.c_int32
            assert a is want or (want is not ctypes.c_void_p and a._type_ == want._type_ and getattr(a, "_length_", 0) == getattr(want, "_length_", 0)), (name, p, a)
    assert os.path.exists(os.path.join(REPO, "treelearn_amd", "csrc", "tl_las.hip"))
