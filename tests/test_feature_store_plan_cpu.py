"""CPU: the host half of the feature stores (include/tdnnf_hip.h, "FEATURE STORES"; tdnn-f_nas_amd/csrc/feature_store_plan.h).
hipabi.FeatureStore.pack / .layout -- the functions an append uses, no device, no handle -- equal the numpy statement
(tests/feature_store_ref.py): format 1 transposed with its p0..p3 computed, an utterance of 13 x 5 = 65 bytes followed by one that starts at
the next 16-byte boundary, 64-bit offsets where the codes pass 2^32 bytes; the compression of float matrices; every refusal by name.  The
feature archive reader hands over the codes untouched and the writer returns the file's bytes.  The same header runs as a stand-alone
program under the address and undefined-behaviour sanitizers (tests/feature_store_driver.cc) over the same cases."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import feature_store_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (13, 30, 12)


def cases():
    """(format, feat_dim, items): the GPU tests' utterances, and a few of other shapes"""
    out = []
    for fmt in (1, 2, 3):
        for D in (8, 5):
            out.append((fmt, D, ref.random_items(10 * fmt + D, fmt, D, FRAMES)))
        out.append((fmt, 40, ref.random_items(fmt, fmt, 40, (7, 1, 33))))
        out.append((fmt, 6, ref.random_items(fmt + 3, fmt, 6, (1,))))
    return out


def test_pack_and_layout_are_the_statement(pkg):
    S = pkg.hipabi.FeatureStore
    for fmt, D, items in cases():
        want = ref.packed(items, fmt, D)
        offsets, total = S.layout(fmt, D, [it["rows"] for it in items])
        assert offsets.dtype == np.int64 and np.array_equal(offsets, want["offsets"]) and total == want["device_bytes"], (fmt, D)
        assert (offsets % 16 == 0).all()
        for k, it in enumerate(items):
            got = S.pack(fmt, D, it)
            assert got["codes"].dtype == want["codes"][k].dtype and np.array_equal(got["codes"], want["codes"][k]), (fmt, D, k)
            assert got["min"] == it["min"] and got["range"] == it["range"]
            if fmt == 1:
                assert np.array_equal(got["header"].view(np.int32), want["headers"][k].view(np.int32)), (D, k)
                # transposed: row-major codes out of Kaldi's column-major ones
                assert got["codes"].shape == (it["rows"], D) and got["codes"][it["rows"] - 1, 1] == it["codes"][1, it["rows"] - 1]
            else:
                assert got["header"] is None
    # 13 x 5 bytes = 65: the next utterance begins at 80, and at 144 with two bytes a code
    assert S.layout(1, 5, [13, 30])[0].tolist() == [0, 80, 80 + 160] and S.layout(3, 5, [13, 30])[1] == 240 + 2 * 32
    assert S.layout(2, 5, [13, 30])[0].tolist() == [0, 144, 144 + 304]
    assert S.layout(1, 5, [13, 30])[1] == 240 + 2 * (32 + 16 * 5)
    # codes that pass 2^32 bytes: 64-bit offsets, no memory
    big = [500_000_000, 500_000_000, 13, 1_000_000_000]
    offsets, total = S.layout(2, 5, big)
    want_offsets, want_total = ref.layout(2, 5, big)
    assert np.array_equal(offsets, want_offsets) and total == want_total and offsets[2] == 10_000_000_000 and offsets[3] == 10_000_000_144 and total > 2 ** 34
    assert S.layout(1, 40, [])[1] == 0


def test_compression_is_the_statement(pkg):
    S = pkg.hipabi.FeatureStore
    rng = np.random.default_rng(5)
    for x in (rng.standard_normal((13, 5)).astype(np.float32) * 7, np.full((4, 3), -2.5, np.float32), rng.standard_normal((1, 40)).astype(np.float32)):
        for fmt in (2, 3):
            got, want = S.pack(fmt, x.shape[1], x), ref.compress(x, fmt)
            assert got["codes"].dtype == want["codes"].dtype and np.array_equal(got["codes"], want["codes"]), (x.shape, fmt)
            assert got["min"] == want["min"] and got["range"] == want["range"] and got["header"] is None
    assert S.pack(2, 3, np.full((4, 3), -2.5, np.float32))["range"] == 1.0


def test_every_refusal_names_what_it_refuses(pkg):
    S, Err = pkg.hipabi.FeatureStore, pkg.hipabi.HipAbiError
    item = ref.random_item(np.random.default_rng(0), 1, 13, 5)

    def refused(words, call, *args):
        with pytest.raises(Err) as e:
            call(*args)
        assert "tdnnf error 1:" in str(e.value) and words in str(e.value), str(e.value)

    S.pack(1, 5, item)
    refused("feature_store_pack: item 0 has 5 columns, feat_dim is 8", S.pack, 1, 8, item)
    refused("feature_store_pack: item 0 has 0 rows", S.pack, 1, 5, dict(item, rows=0, codes=np.zeros((5, 0), np.uint8)))
    refused("feature_store_pack: item 0: its min or range is not finite", S.pack, 1, 5, dict(item, min=np.float32("nan")))
    refused("feature_store_pack: item 0: its min or range is not finite", S.pack, 1, 5, dict(item, range=np.float32("inf")))
    refused("feature_store_pack: format 4: a payload is of format 1 (CM), 2 (CM2) or 3 (CM3)", S.pack, 4, 5, dict(item, format=4))
    with pytest.raises(Err, match="item 0 is a payload of format 1, not of format 3"):
        S.pack(3, 5, item)
    x = np.ones((4, 5), np.float32)
    refused("feature_store_compress: format 1 (CM) from float matrices is not built: Kaldi's percentile selection", S.pack, 1, 5, x)
    refused("feature_store_compress: item 0 has 0 rows", S.pack, 2, 5, np.zeros((0, 5), np.float32))
    refused("feature_store_compress: item 0: its min or range is not finite", S.pack, 2, 5, np.asarray([[1.0, np.inf]], np.float32))
    refused("feature_store_compress: item 0: its min or range is not finite", S.pack, 3, 5, np.asarray([[-3e38, 3e38]], np.float32))
    refused("feature_store_layout: utterance 1 has 0 frames", S.layout, 1, 5, [13, 0])
    refused("feature_store_layout: format 0: a store holds format 1 (CM), 2 (CM2) or 3 (CM3)", S.layout, 0, 5, [13])
    refused("feature_store_layout: feat_dim 0 must be positive", S.layout, 1, 0, [13])
    refused("feature_store_layout: 2147483648 frames in all: a store holds at most 2^31 - 1", S.layout, 1, 5, [2 ** 30, 2 ** 30])
    with pytest.raises(Err, match="an item of 13 x 5 with 64 codes"):
        S.pack(1, 5, dict(item, codes=np.zeros(64, np.uint8)))
    with pytest.raises(Err, match="an item of 5 columns with 16 percentiles"):
        S.pack(1, 5, dict(item, percentiles=np.zeros(16, np.uint16)))


def test_feature_archives_keep_the_codes(pkg, tmp_path):
    E = pkg.egs
    rng = np.random.default_rng(3)
    full = rng.standard_normal((4, 3)).astype(np.float32)
    double = rng.standard_normal((2, 5))
    items = [("cm", ref.random_item(rng, 1, 13, 5)), ("cm2", ref.random_item(rng, 2, 9, 8)), ("cm3", ref.random_item(rng, 3, 6, 4))]
    blob = b"full \0BFM " + struct.pack("<bibi", 4, 4, 4, 3) + full.tobytes()
    blob += b"".join(ref.archive_bytes(k, it) for k, it in items)
    blob += b"double \0BDM " + struct.pack("<bibi", 4, 2, 4, 5) + double.astype("<f8").tobytes()
    path = tmp_path / "feats.ark"
    path.write_bytes(blob)
    got = list(E.read_feature_archive(path))
    assert [k for k, _ in got] == ["full", "cm", "cm2", "cm3", "double"]
    assert got[0][1].dtype == np.float32 and np.array_equal(got[0][1], full) and np.array_equal(got[4][1], double.astype(np.float32))
    for (_, want), (_, it) in zip(items, got[1:4]):
        assert set(it) == set(want) and it["format"] == want["format"] and (it["rows"], it["cols"]) == (want["rows"], want["cols"])
        assert it["min"] == want["min"] and it["range"] == want["range"] and it["min"].dtype == np.float32
        assert it["codes"].dtype == want["codes"].dtype and it["codes"].shape == want["codes"].shape and np.array_equal(it["codes"], want["codes"])
        if want["format"] == 1:
            assert it["percentiles"].dtype == np.uint16 and np.array_equal(it["percentiles"], want["percentiles"])
    # the writer returns the file's bytes; the float writer stays infer.write_matrix_archive
    back = tmp_path / "back.ark"
    E.write_feature_archive(back, got[1:4])
    assert back.read_bytes() == b"".join(ref.archive_bytes(k, it) for k, it in items)
    pkg.infer.write_matrix_archive(back, [got[0]])
    assert back.read_bytes() == blob[:len(b"full \0BFM ") + 10 + full.nbytes]
    assert [k for k, _ in E.read_feature_archive(back)] == ["full"]
    # the writer refuses what is no item, by ValueError as the reader does
    for bad, words in ((dict(items[0][1], codes=np.zeros(64, np.uint8)), "entry cm is 13 x 5 with 64 codes"),
                       (dict(items[0][1], percentiles=np.zeros(16, np.uint16)), "entry cm has 5 columns and 16 percentiles"),
                       (dict(items[1][1], format=4), "format 4")):
        with pytest.raises(ValueError, match=words):
            E.write_feature_archive(back, [("cm", bad)])
    with pytest.raises(ValueError, match="a key without spaces"):
        E.write_feature_archive(back, [("two words", items[0][1])])
    # a truncated file and an entry that is no matrix are refused
    path.write_bytes(blob[:40])
    with pytest.raises(ValueError, match="unexpected end of file"):
        list(E.read_feature_archive(path))
    path.write_bytes(b"k \0BSM \x04")
    with pytest.raises(ValueError, match="not a matrix"):
        list(E.read_feature_archive(path))


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "feature_store_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "feature_store_driver.cc"), "-o", str(exe)])
    all_cases = cases()
    rng = np.random.default_rng(8)
    floats = [(fmt, rng.standard_normal((r, c)).astype(np.float32) * 5) for fmt in (2, 3) for r, c in ((13, 5), (1, 8), (30, 40))]
    floats.append((2, np.full((3, 4), 1.5, np.float32)))
    ints = lambda a: " ".join("%d" % x for x in np.asarray(a).reshape(-1)) + "\n"
    with open(tmp_path / "cases.txt", "w") as f:
        for fmt, D, items in all_cases:
            want = ref.packed(items, fmt, D)
            f.write("store %d %d %d %d\n" % (fmt, D, len(items), want["device_bytes"]))
            f.write(ints(want["offsets"]))
            for k, it in enumerate(items):
                f.write("%d %d %d\n" % (it["rows"], np.float32(it["min"]).view(np.int32), np.float32(it["range"]).view(np.int32)))
                if fmt == 1:
                    f.write(ints(it["percentiles"]) + ints(want["headers"][k].view(np.int32)))
                f.write(ints(it["codes"]) + ints(want["codes"][k]))
        for fmt, x in floats:
            want = ref.compress(x, fmt)
            f.write("float %d %d %d %d %d\n" % (fmt, x.shape[0], x.shape[1], want["min"].view(np.int32), want["range"].view(np.int32)))
            f.write(ints(x.view(np.int32)) + ints(want["codes"]))
    out = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failures" and lines[0] == "cases: %d stores, %d float matrices" % (len(all_cases), len(floats)) and len(all_cases) >= 12, out.stdout
    assert sum(line.startswith("refusal: driver: ") for line in lines) == 14, out.stdout
