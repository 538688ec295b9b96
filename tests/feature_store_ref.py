"""The feature stores (include/tdnnf_hip.h, "FEATURE STORES") stated from their definition in plain numpy float32, one rounding an
operation, in the order the header writes: the value of a code of Kaldi's three CompressedMatrix formats (decode), the writer's
compression rule (compress), what a store holds of a list of items (packed: 64-bit code offsets, header floats, row-major codes,
device_bytes), an archive entry's bytes (archive_bytes), and a maker of fixtures that draws codes and headers DIRECTLY -- every branch and
both ends of every format are hit in every utterance, which compressing random floats would not guarantee.
An item is the dict hipabi.FeatureStore.append takes and egs.read_feature_archive yields: {"format", "min", "range", "rows", "cols", "codes"
[, "percentiles"]}, codes in Kaldi's order (format 1: uint8 [cols, rows] column-major, 2: uint16 [rows, cols], 3: uint8 [rows, cols])."""
import numpy as np

F = np.float32
K16, K8 = F(1.0) / F(65535.0), F(1.0) / F(255.0)
TOKENS = {1: b"CM", 2: b"CM2", 3: b"CM3"}
EDGE_CODES = {1: (0, 64, 65, 192, 193, 255), 2: (0, 65535), 3: (0, 255)}


def decode(item):
    """float32 [rows, cols]: the value of every code"""
    mn, rg, fmt = F(item["min"]), F(item["range"]), item["format"]
    if fmt == 2:
        return mn + rg * K16 * np.asarray(item["codes"], np.uint16).astype(F)
    if fmt == 3:
        return mn + rg * K8 * np.asarray(item["codes"], np.uint8).astype(F)
    p = mn + rg * K16 * np.asarray(item["percentiles"], np.uint16).astype(F)  # [cols, 4]
    b = np.asarray(item["codes"], np.uint8).T.astype(np.int32)  # [rows, cols]
    p0, p1, p2, p3 = (p[None, :, i] for i in range(4))
    low = p0 + (p1 - p0) * b.astype(F) * (F(1.0) / F(64.0))
    mid = p1 + (p2 - p1) * (b - 64).astype(F) * (F(1.0) / F(128.0))
    high = p2 + (p3 - p2) * (b - 192).astype(F) * (F(1.0) / F(63.0))
    out = np.where(b <= 64, low, np.where(b <= 192, mid, high))
    assert out.dtype == F
    return out


def compress(matrix, fmt):
    """the writer's rule (kTwoByteAuto, or the same over 8 bits): an item of format 2 or 3"""
    x = np.asarray(matrix, F)
    levels, kind = (F(65535.0), np.uint16) if fmt == 2 else (F(255.0), np.uint8)
    mn, mx = x.min(), x.max()
    if not mx > mn:
        mx = mn + F(1.0)
    rg = F(mx - mn)
    f = (x - mn) / rg
    codes = np.minimum(levels, np.maximum(F(0.0), f * levels + F(0.499))).astype(kind)  # (the cast truncates)
    return dict(format=fmt, min=F(mn), range=rg, rows=x.shape[0], cols=x.shape[1], codes=codes)


def code_width(fmt):
    return 2 if fmt == 2 else 1


def layout(fmt, feat_dim, frames):
    """(offsets int64 [U + 1], device_bytes): the header's closed form, in Python integers"""
    offsets = [0]
    for f in frames:
        offsets.append(offsets[-1] + (int(f) * feat_dim * code_width(fmt) + 15) // 16 * 16)
    return np.asarray(offsets, np.int64), offsets[-1] + len(frames) * (32 + (16 * feat_dim if fmt == 1 else 0))


def packed(items, fmt, feat_dim):
    """what a store of these items holds: dict(offsets, device_bytes, headers [U] of float32 [feat_dim, 4] or None, codes [U] row-major)"""
    assert all(it["format"] == fmt and it["cols"] == feat_dim for it in items)
    offsets, total = layout(fmt, feat_dim, [it["rows"] for it in items])
    headers = [(F(it["min"]) + F(it["range"]) * K16 * np.asarray(it["percentiles"], np.uint16).astype(F)) if fmt == 1 else None for it in items]
    codes = [np.ascontiguousarray(np.asarray(it["codes"]).T if fmt == 1 else np.asarray(it["codes"])) for it in items]
    return dict(offsets=offsets, device_bytes=total, headers=headers, codes=codes)


def matrix_bytes(item):
    """a CompressedMatrix as an archive holds it: token, global header, [percentiles,] codes"""
    out = TOKENS[item["format"]] + b" " + np.asarray([item["min"], item["range"]], "<f4").tobytes() + np.asarray([item["rows"], item["cols"]], "<i4").tobytes()
    if item["format"] == 1:
        out += np.asarray(item["percentiles"], "<u2").tobytes()
    return out + np.asarray(item["codes"], "<u2" if item["format"] == 2 else np.uint8).tobytes()


def archive_bytes(key, item):
    return key.encode() + b" \0B" + matrix_bytes(item)


def random_item(rng, fmt, rows, cols):
    """codes and headers drawn directly; the format's edge codes are planted at random places of every item (rows * cols >= 6)"""
    mn, rg = F(rng.uniform(-20, 5)), F(rng.uniform(0.5, 40))
    item = dict(format=fmt, min=mn, range=rg, rows=rows, cols=cols)
    kind, top = (np.uint16, 65536) if fmt == 2 else (np.uint8, 256)
    codes = rng.integers(0, top, size=rows * cols).astype(kind)
    edges = EDGE_CODES[fmt]
    assert rows * cols >= len(edges)
    codes[rng.choice(rows * cols, size=len(edges), replace=False)] = edges
    if fmt == 1:
        item["percentiles"] = np.sort(rng.integers(0, 65536, size=(cols, 4)), axis=1).astype(np.uint16)  # non-decreasing
        item["codes"] = codes.reshape(cols, rows)
    else:
        item["codes"] = codes.reshape(rows, cols)
    assert set(edges) <= set(item["codes"].reshape(-1).tolist())
    return item


def random_items(seed, fmt, feat_dim, frames):
    rng = np.random.default_rng(seed)
    return [random_item(rng, fmt, f, feat_dim) for f in frames]
