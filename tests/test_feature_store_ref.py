"""CPU: the numpy statement of the feature stores (tests/feature_store_ref.py) is the decompression the library already ships.  decode has
the BITS of egs.Reader(...).input() on example streams assembled here, field by field as tests/test_egs_io.py assembles them, around CM, CM2
and CM3 matrices whose codes and headers are drawn directly (every branch, both ends); compress(X, 2) then decode has the bits of what
Writer.write(compress=True) writes and the reader reads back.  So the statement is a valid yardstick for the device decode, and the header
that egs_io.hip now shares with the kernels (csrc/feature_code_value.h) left the reader's results where they were."""
import numpy as np
import pytest

from tests import feature_store_ref as ref
from tests.test_egs_io import _minibatch, eg_bytes, two_frame_fst


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_decode_has_the_bits_of_the_egs_reader(pkg, tmp_path, fmt):
    rng = np.random.default_rng(fmt)
    items = [ref.random_item(rng, fmt, rows, cols) for rows, cols in ((9, 5), (13, 8), (2, 3), (40, 40))]
    # every 8-bit code against one header; a sweep of the 16-bit codes
    if fmt == 2:
        sweep = dict(format=2, min=np.float32(-7.25), range=np.float32(19.5), rows=257, cols=255, codes=np.arange(65535, dtype=np.uint16).reshape(257, 255))
    else:
        sweep = dict(format=fmt, min=np.float32(-7.25), range=np.float32(19.5), rows=256, cols=3)
        sweep["codes"] = np.tile(np.arange(256, dtype=np.uint8), (3, 1)) if fmt == 1 else np.tile(np.arange(256, dtype=np.uint8)[:, None], (1, 3))
        if fmt == 1:
            sweep["percentiles"] = np.asarray([[0, 9000, 41000, 65535], [100, 100, 100, 100], [5, 6, 60000, 60001]], np.uint16)
    items.append(sweep)
    fst = two_frame_fst()
    path = tmp_path / "hand.ark"
    path.write_bytes(b"".join(eg_bytes("k%d" % i, ref.matrix_bytes(it), it["rows"], -2, fst, 2, 10) for i, it in enumerate(items)))
    egs = list(pkg.egs.Reader(path))
    assert len(egs) == len(items)
    for it, eg in zip(items, egs):
        got, t0 = eg.input()
        want = ref.decode(it)
        assert t0 == -2 and got.shape == want.shape == (it["rows"], it["cols"]) and want.dtype == np.float32
        assert np.array_equal(bits(got), bits(want)), (fmt, it["rows"], it["cols"], np.abs(got - want).max())
    if fmt == 1:  # the statement's own edges: the pieces meet at the percentiles
        d = ref.decode(sweep)
        p = ref.F(-7.25) + ref.F(19.5) * ref.K16 * sweep["percentiles"].astype(np.float32)
        assert np.array_equal(d[0], p[:, 0])
        for code, i in ((64, 1), (192, 2), (255, 3)):  # (p0 + (p1 - p0) is p1 up to its roundings)
            np.testing.assert_allclose(d[code], p[:, i], rtol=0, atol=1e-5)
        assert (np.diff(d, axis=0) >= -1e-5).all()


def test_compress_then_decode_has_the_bits_of_the_writer_read_back(pkg, tmp_path):
    E = pkg.egs
    sup, feats, ivs, rows = _minibatch(pkg, B=3, T=8, P=20, feat_dim=6)
    feats[1] = np.full_like(feats[1], 2.5)  # a constant matrix: max = min + 1
    path = tmp_path / "cm2.ark"
    with E.Writer(path) as w:
        for b in range(3):
            w.write("utt%d" % b, feats[b], -5, E.sequence_of(sup, b), 20, ivector=ivs[b], compress=True)
    for b, eg in enumerate(E.Reader(path)):
        got, _ = eg.input()
        item = ref.compress(feats[b], 2)
        assert item["codes"].dtype == np.uint16 and np.array_equal(bits(got), bits(ref.decode(item))), b
    assert ref.compress(feats[1], 2)["range"] == 1.0 and not ref.compress(feats[1], 2)["codes"].any()
    # the codes themselves: the archive's bytes hold the statement's matrix
    blob = path.read_bytes()
    for b in range(3):
        assert ref.matrix_bytes(ref.compress(feats[b], 2)) in blob, b
    # 8 bits: both ends are reached, every value within half a step
    x = feats[0]
    item = ref.compress(x, 3)
    assert item["codes"].dtype == np.uint8 and item["codes"].min() == 0 and item["codes"].max() == 255
    assert np.abs(ref.decode(item) - x).max() <= 0.502 * float(item["range"]) / 255
