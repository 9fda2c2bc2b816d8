"""GPU tests of the LAS record passes (csrc/tl_las.hip) and of the reader / writer built on them (treelearn_amd/util/las.py)
against the numpy restatement of tests/las_restatement.py.

Bounds.  Decoding is compared bit for bit (two float64 roundings in a fixed order, integer label logic) and encoding byte for byte
(subtract, divide, round half to even; integer colours and extremes).  A round trip write -> read is held to
|d| <= scale / 2 + 8 * 2^-52 * max(|x|, |offset|, |x - offset|): rint moves the quotient by at most 1/2, and the five roundings involved
(the subtraction, the division, the integer-to-double product, the addition, and the f64 mean behind the offset, which both sides share
and which therefore drops out) each contribute at most 2^-53 relative to an operand no larger than that maximum; 8 covers them with the
division's amplification by scale / scale."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import las_cases as cases
import las_restatement as ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)
CREATED = (17, 2031)
# (record length, point format, treeID type or None): 20 .. 67 + 8 are read by both paths in turn, 700 only by the plain one
LAYOUTS = ((20, 0, None), (26, 2, None), (28, 1, None), (34, 3, None), (35, 3, 1), (38, 3, 5), (39, 8, 2), (67 + 8, 10, 10), (700, 6, 8))
TID_VALUES = {1: [0, 1, 255], 2: [0, -128, 127], 3: [0, 65535, 300], 4: [0, -32768, 12], 5: [0, 2 ** 32 - 1, 70000], 6: [0, -2 ** 31, 5],
              7: [0, 2 ** 64 - 1, 2 ** 63 + 1025, 2 ** 53 + 1], 8: [0, -2 ** 63, 2 ** 53 + 1, -7], 9: [0.0, 2.5, -3.0, 1e10], 10: [0.0, 2.5, -3.0, 1e300]}
CLASS_BYTES = [0, 1, 2, 4, 34, 0b10100010, 0b11100001, 0xff]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def paths_of(record_length):
    return ("auto", "plain", "staged") if record_length <= 128 else ("auto", "plain")


def random_file(n, record_length, fmt, tid_type, seed, scale=(0.001, 0.01, 1e-4), offset=(512345.678, 5412345.25, 312.5)):
    """A LAS 1.2 / 1.4 file of n records of the given length: random bytes everywhere, then random i32 X Y Z (the extremes among them), a
    class byte and the treeID values of TID_VALUES; the treeID sits right after the base block."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (n, record_length), dtype=np.uint8)
    xyz = rng.integers(-2 ** 31, 2 ** 31, (n, 3)).astype("<i4")
    xyz[0] = [2 ** 31 - 1, -(2 ** 31 - 1), -2 ** 31]
    raw[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    raw[:, 15 if fmt <= 5 else 16] = rng.choice(CLASS_BYTES, n)
    vlrs = []
    base = cases.BASE[fmt]
    if tid_type is not None:
        dt = np.dtype(ref.EXTRA_TYPES[tid_type])
        vals = np.array(TID_VALUES[tid_type], dtype=dt)[rng.integers(0, len(TID_VALUES[tid_type]), n)]
        raw[:, base:base + dt.itemsize] = vals.view(np.uint8).reshape(n, dt.itemsize)
        vlrs = [cases.extra_vlr(("treeID", tid_type, 0))]
    return cases.las_file((1, 4) if fmt >= 6 else (1, 2), fmt, [raw.tobytes()], scale, offset, vlrs, count=n, record_length=record_length)


def check_read(tmp_path, name, buf, **kw):
    from treelearn_amd.util.las import read_las
    p = tmp_path / name
    p.write_bytes(buf)
    want = ref.read(buf)
    h = ref.parse(buf)
    for mode in paths_of(h["record_length"]):
        got = read_las(str(p), path_mode=mode, **kw)
        assert got.dtype == np.float64 and got.shape == want.shape, (name, mode, got.shape, want.shape)
        same = bits(got) == bits(want)
        assert same.all(), (name, mode, int((~same).sum()), got[~same.all(1)][:3], want[~same.all(1)][:3])
    return want


def test_hand_cases_read_bit_for_bit(tmp_path):
    for name, (buf, want, _) in cases.good_cases().items():
        got = check_read(tmp_path, name + ".las", buf)
        assert np.array_equal(got, want), name                                   # the restatement and the hand values agree (also a host test)


@pytest.mark.parametrize("record_length,fmt,tid_type", LAYOUTS)
def test_decode_row_counts_and_record_lengths(tmp_path, record_length, fmt, tid_type):
    for n in ROW_COUNTS:
        want = check_read(tmp_path, f"r{record_length}_{n}.las", random_file(n, record_length, fmt, tid_type, seed=n))
        assert want.shape == (n, 3 if tid_type is None else 4)
    if record_length > 128:
        from treelearn_amd import _hip
        from treelearn_amd.util import las
        h = las.read_header(str(tmp_path / f"r{record_length}_1.las"))
        rec = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        out = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError, match="tl_las_decode"):                 # a record too long to stage is refused, not staged
            las.decode_records(rec, 1, h, out, path="staged")
        assert _hip.TL_ERR_UNSUPPORTED == -3


@pytest.mark.parametrize("tid_type", range(1, 11))
def test_decode_every_tree_id_type(tmp_path, tid_type):
    width = np.dtype(ref.EXTRA_TYPES[tid_type]).itemsize
    want = check_read(tmp_path, f"t{tid_type}.las", random_file(257, 34 + width, 3, tid_type, seed=tid_type))
    assert want.shape == (257, 4) and set(np.unique(want[:, 3])) >= {0.0, -1.0}   # both rules met


def test_decode_in_chunks_and_on_device(tmp_path):
    from treelearn_amd.util.las import read_las
    buf = random_file(257, 39, 8, 2, seed=3)
    want = check_read(tmp_path, "chunks.las", buf, chunk_records=100)
    dev = read_las(str(tmp_path / "chunks.las"), chunk_records=1, device_out=True)
    assert dev.is_cuda and (bits(dev.cpu().numpy()) == bits(want)).all()


def test_decode_is_not_contracted(tmp_path):
    """Random i32 X against offset 512345.678: a fused multiply-add rounds about 30 % of these values differently."""
    buf = random_file(1025, 38, 3, 5, seed=11, scale=(0.001,) * 3, offset=(512345.678,) * 3)
    want = check_read(tmp_path, "fma.las", buf)
    X = ref.field(buf, ref.parse(buf), 0, "<i4")
    fused = ref.fma_read_x(X, 0.001, 512345.678)
    assert 0.1 < np.mean(fused != want[:, 0]) < 0.6                              # the comparison above would have seen it


# ---------------------------------------------------------------------------------------------------------------- encode
def cloud(n, seed, centre=(512345.678, 5412345.25, 312.5)):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-60, 60, (n, 3)) + np.asarray(centre)
    labels = rng.integers(-1, 6, n).astype(np.int64)
    labels[rng.integers(0, n, max(1, n // 8))] = 2 ** 40 + 12345                  # only the low 32 bits are written
    return xyz, labels


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("ordered", [False, True])
def test_encode_byte_for_byte(dtype, stride, ordered):
    from treelearn_amd.util import las
    for n in (1, 255, 256, 257, 1025):
        xyz, labels = cloud(n, n, centre=(10.0, -20.0, 3.0))
        xyz = xyz.astype(dtype)
        offset = xyz.astype(np.float64).mean(0)
        order = np.random.default_rng(n + 1).permutation(n)[: max(1, (2 * n) // 3)] if ordered else None
        src = torch.from_numpy(xyz).cuda()
        if stride == 4:
            src = torch.cat([src, torch.full((n, 1), 7.0, dtype=src.dtype, device="cuda")], 1)[:, :3]
            assert src.stride(0) == 4
        sel = slice(None) if order is None else order
        want = ref.records(xyz[sel], labels[sel], offset=offset)
        rec, ext = las.encode_records(src, labels, order=order, offset=offset)
        assert rec.dtype == torch.uint8 and rec.cpu().numpy().tobytes() == want.tobytes(), n
        assert ext.dtype == np.int32 and ext.shape == (1, 6) and np.array_equal(ext[0], ref.extremes(want)), n


def test_encode_ties_negatives_and_limits():
    from treelearn_amd.util import las
    k = np.arange(-40, 41, dtype=np.float64)
    x = (k + 0.5) * 0.5                                                          # with scale 0.5 the quotient is k + 0.5 exactly: both parities, both signs
    xyz = np.stack([x, -x, x + 0.25], 1)
    labels = np.arange(len(k), dtype=np.int64) - 40
    want = ref.records(xyz, labels, scale=(0.5,) * 3)
    X = np.ascontiguousarray(want[:, :4]).view("<i4").reshape(-1)
    assert np.array_equal(X, np.rint(k + 0.5).astype(np.int32)) and (X % 2 == 0).all()
    lim = np.array([[2147483.647, -2147483.648, 0.0], [-2147483.648, 2147483.647, -0.0004]])
    rec, _ = las.encode_records(xyz, labels, scale=(0.5,) * 3)
    assert rec.cpu().numpy().tobytes() == want.tobytes()
    rec, ext = las.encode_records(lim, [1, 2])
    assert rec.cpu().numpy().tobytes() == ref.records(lim, [1, 2]).tobytes()
    assert ext[0].tolist() == [-2 ** 31, -2 ** 31, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0]
    # the hand bytes
    rec, ext = las.encode_records(cases.HAND_COORDS, cases.HAND_LABELS)
    assert rec.cpu().numpy().tobytes() == cases.HAND_RECORDS and ext[0].tolist() == cases.HAND_EXTREMES


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2147483.648, -2147483.649])
def test_encode_refuses_what_does_not_fit(tmp_path, bad):
    from treelearn_amd.util import las
    xyz, labels = cloud(300, 1, centre=(0.0, 0.0, 0.0))
    xyz[257, 1] = bad
    with pytest.raises(ValueError):
        ref.records(xyz, labels)
    with pytest.raises(ValueError, match="nothing was written"):
        las.encode_records(xyz, labels)
    p = tmp_path / "never.las"
    with pytest.raises(ValueError, match="nothing was written"):
        las.write_las(str(p), xyz, labels, use_offset=False)
    assert not p.exists()
    with pytest.raises(ValueError, match="nothing was written"):
        las.write_las_segments([str(p)], xyz, labels, np.arange(300), [0, 300])
    assert not p.exists()


def test_encode_segments_table_and_order_independence():
    from treelearn_amd.util import las
    n = 1 + 64 + 257
    starts = np.array([0, 1, 65, 65, n])                                         # segments of 1, 64, 0 and 257 rows
    xyz, labels = cloud(400, 9, centre=(0.0, 0.0, 0.0))
    order = np.random.default_rng(2).permutation(400)[:n]
    want = ref.records(xyz[order], labels[order])
    want_ext = np.stack([ref.extremes(want[a:b]) for a, b in zip(starts[:-1], starts[1:])])
    assert want_ext[2].tolist() == [2 ** 31 - 1] * 3 + [-2 ** 31] * 3
    runs = []
    for run in range(2):                                                         # two runs
        rec, ext = las.encode_records(xyz, labels, order=order, starts=starts)
        runs.append(rec.cpu().numpy().tobytes())
        assert runs[-1] == want.tobytes() and ext.dtype == np.int32 and np.array_equal(ext, want_ext), run
    # the same cloud with its rows stored in another order, addressed through a matching `order`: the same bytes, the same table
    perm = np.random.default_rng(3).permutation(400)
    inv = np.empty(400, np.int64); inv[perm] = np.arange(400)
    rec, ext = las.encode_records(xyz[perm], labels[perm], order=inv[order], starts=starts)
    assert rec.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(ext, want_ext)
    # rows shuffled inside every segment: the same records per segment as a set, the same table
    shuffled = np.concatenate([np.random.default_rng(4).permutation(order[a:b]) for a, b in zip(starts[:-1], starts[1:])])
    rec, ext = las.encode_records(xyz, labels, order=shuffled, starts=starts)
    got = rec.cpu().numpy().reshape(-1, 38)
    for a, b in zip(starts[:-1], starts[1:]):
        assert sorted(r.tobytes() for r in got[a:b]) == sorted(r.tobytes() for r in want[a:b])
    assert np.array_equal(ext, want_ext)


# ---------------------------------------------------------------------------------------------------------------- files
def bound(x, offset, scale=0.001):
    return scale / 2 + 8 * 2.0 ** -52 * np.maximum(np.maximum(np.abs(x), np.abs(offset)), np.abs(x - offset))


def box_encloses(h, pts):
    return (np.asarray(h.mins) <= pts[:, :3].min(0)).all() and (pts[:, :3].max(0) <= np.asarray(h.maxs)).all()


@pytest.mark.parametrize("use_offset", [True, False])
def test_write_then_read(tmp_path, use_offset):
    from treelearn_amd.util import las
    xyz, labels = cloud(1025, 21) if use_offset else cloud(1025, 22, centre=(100.0, -200.0, 30.0))
    p = str(tmp_path / "rt.las")
    las.write_las(p, xyz, labels, use_offset=use_offset, created=CREATED)
    h = las.read_header(p)
    offset = np.asarray(h.offset)
    assert np.array_equal(offset, xyz.mean(0) if use_offset else np.zeros(3))
    assert open(p, "rb").read() == ref.write(xyz, labels, offset, CREATED)       # the whole file, header included
    assert (h.version, h.point_format, h.record_length, h.count, h.offset_to_points) == ((1, 2), 3, 38, 1025, 473)
    back = las.read_las(p)
    d = np.abs(back[:, :3] - xyz)
    print(f"round trip: max |d| {d.max():.3e} against a bound of {bound(xyz, offset).min():.3e}")
    assert (d <= bound(xyz, offset)).all()
    assert box_encloses(h, back)
    want = np.where(labels == 0, 0, labels & 0xffffffff).astype(np.float64)        # label -1 comes back as 4294967295 (deviations)
    assert np.array_equal(back[:, 3], want) and np.array_equal(back[labels >= 0, 3] % 2 ** 32, (labels[labels >= 0] % 2 ** 32).astype(np.float64))
    small = labels.copy(); small[small > 100] = 3
    las.write_las(p, torch.from_numpy(xyz.astype(np.float32)).cuda(), torch.from_numpy(small).cuda(), use_offset=use_offset)       # device input, f32
    back = las.read_las(p)
    assert np.array_equal(back[small >= 0, 3], small[small >= 0].astype(np.float64))
    x32 = xyz.astype(np.float32).astype(np.float64)
    assert (np.abs(back[:, :3] - x32) <= bound(x32, np.asarray(las.read_header(p).offset))).all()
    las.write_las(p, np.zeros((0, 3)), np.zeros(0, np.int64), created=CREATED)                                                     # an empty cloud
    assert open(p, "rb").read() == ref.write(np.zeros((0, 3)), np.zeros(0, np.int64), np.zeros(3), CREATED) and las.read_las(p).shape == (0, 4)


def test_save_results_las(tmp_path):
    from treelearn_amd.util import las
    from treelearn_amd.util.segment import CATEGORIES, save_results
    rng = np.random.default_rng(31)
    n, T = 3000, 6
    coords = rng.uniform(-40, 40, (n, 3)) + np.array([512345.678, 5412345.25, 312.5])
    labels = rng.integers(0, T + 1, n).astype(np.int64)
    labels[:3] = [T, 0, 1]
    cats = np.array([0, 1, 2, 0, 1, 2])
    result = dict(coords=coords, labels=labels, categories=cats)
    save_results(result, str(tmp_path / "a"), "plot", ["las", "npz"])
    save_results(result, str(tmp_path / "b"), "plot", ["npz"])
    full = las.read_las(str(tmp_path / "a" / "full_forest" / "plot.las"))
    h = las.read_header(str(tmp_path / "a" / "full_forest" / "plot.las"))
    with np.load(tmp_path / "a" / "full_forest" / "plot.npz") as z:
        assert (np.abs(full[:, :3] - z["points"]) <= bound(z["points"], np.asarray(h.offset))).all()
        assert np.array_equal(full[:, 3], z["labels"])
    assert h.count == n and box_encloses(h, full) and np.array_equal(np.asarray(h.offset), coords.mean(0))
    trees = tmp_path / "a" / "individual_trees"
    found = sorted(str(p.relative_to(trees)) for p in trees.rglob("*.las"))
    assert found == sorted(["non_trees.las"] + [os.path.join(CATEGORIES[cats[i - 1]], f"{i}.las") for i in range(1, T + 1)])
    assert not list(trees.rglob("*.npz"))
    for rel in found:
        p = str(trees / rel)
        i = 0 if rel == "non_trees.las" else int(os.path.basename(rel)[:-4])
        h, got = las.read_header(p), las.read_las(p)
        with np.load(str(tmp_path / "b" / "individual_trees" / rel)[:-4] + ".npz") as z:
            want = z["points"]
            assert np.array_equal(z["labels"], np.full(len(want), float(i)))
        assert h.count == len(want) == int((labels == i).sum()) and h.offset == (0.0, 0.0, 0.0), rel
        assert np.array_equal(got[:, 3], np.full(len(want), float(i))), rel
        assert (np.abs(got[:, :3] - want) <= bound(want, 0.0)).all(), rel
        assert box_encloses(h, got), rel


def test_inventory_cli_reads_las(tmp_path):
    """`inventory --forest cloud.las` gives the CSV of the same cloud from .npy (the cloud the file holds: coordinates on its 1 mm grid)."""
    from treelearn_amd.util import inventory, las
    rng = np.random.default_rng(41)
    parts = []
    for t in range(1, 4):                                                        # three stems with a blob on top, and some ground
        z = rng.uniform(0, 12, 400)
        r = np.where(z < 8, 0.15, 1.5) * np.sqrt(rng.uniform(0.8, 1, 400))
        a = rng.uniform(0, 2 * np.pi, 400)
        parts.append(np.stack([6.0 * t + r * np.cos(a), -3.0 * t + r * np.sin(a), z, np.full(400, float(t))], 1))
    parts.append(np.concatenate([rng.uniform(0, 25, (500, 2)) * [1, -1], rng.uniform(-0.1, 0.1, (500, 1)), np.zeros((500, 1))], 1))
    data = np.concatenate(parts) + [500000.0, 5400000.0, 300.0, 0.0]
    las.write_las(str(tmp_path / "cloud.las"), data[:, :3], data[:, 3].astype(np.int64))
    held = las.read_las(str(tmp_path / "cloud.las"))
    assert held.shape == data.shape and np.array_equal(held[:, 3], data[:, 3])
    np.save(tmp_path / "cloud.npy", held)
    assert inventory.main(["--forest", str(tmp_path / "cloud.npy"), "--out", str(tmp_path / "npy.csv")]) == 0
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "treelearn_amd.util.inventory", "--forest", str(tmp_path / "cloud.las"),
                        "--out", str(tmp_path / "las.csv")], capture_output=True, text=True, cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO))
    assert p.returncode == 0 and "3 trees" in p.stdout, (p.stdout[-500:], p.stderr[-2000:])
    assert (tmp_path / "las.csv").read_bytes() == (tmp_path / "npy.csv").read_bytes()
    assert len((tmp_path / "las.csv").read_text().splitlines()) == 4
