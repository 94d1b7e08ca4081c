"""Helpers of tests/test_build_extend.py: builders seeded from stored databases, the section compare, stream read-back, and the byte offsets
of a stored file's first table item and pattern headers (for the files the refusal tests damage)."""
import struct

import numpy as np

import build_cases as BC


def read(path):
    with open(path, "rb") as f:
        return f.read()


def build(K, k, f, names, lists, calls=None, alphabet="nt", start=0.0):
    """add_kmers in calls of the given sizes (None: one call), finish -> (HostDB, stats)"""
    b = K.Builder(k, f, start, alphabet)
    try:
        at = 0
        for n in (calls or [len(names)]):
            b.add_kmers(names[at: at + n], lists[at: at + n])
            at += n
        assert at == len(names)
        return b.finish(), b.stats()
    finally:
        b.close()


def build_file(K, k, f, names, lists, path, **kw):
    h, st = build(K, k, f, names, lists, **kw)
    h.store(path)
    h.close()
    return read(path), st


def extend(K, old_path, names, lists, calls=None):
    """HostDB(old_path) -> Builder.from_db -> add_kmers in calls -> finish; the loaded database is closed before the first add"""
    old = K.HostDB(old_path)
    b = K.Builder.from_db(old)
    try:
        seed = b.seed_stats()
        assert (seed["samples"], seed["patterns"]) == (old.N, int(old.view.contents.n_patterns))
        old.close()
        at = 0
        for n in (calls or ([len(names)] if names else [])):
            b.add_kmers(names[at: at + n], lists[at: at + n])
            at += n
        assert at == len(names)
        return b.finish(), b.stats(), seed
    finally:
        b.close()


def extend_file(K, old_path, names, lists, path, calls=None):
    h, st, seed = extend(K, old_path, names, lists, calls)
    h.store(path)
    h.close()
    return read(path), st


def same_sections(got, want, tables="bytes"):
    """header + samples equal, patterns equal under the section compare; tables byte for byte, or by content and well formed"""
    x, y = BC.split_db(got), BC.split_db(want)
    assert x["head"] == y["head"], "header / sample table differ"
    assert x["P"] == y["P"]
    assert BC.masked_patterns(x["patterns_raw"]) == BC.masked_patterns(y["patterns_raw"]), "pattern sections differ"
    if tables == "bytes":
        assert x["tables_raw"] == y["tables_raw"], "hashtable sections differ"
    else:
        assert x["n_buckets"] == y["n_buckets"]
        assert BC.table_sets(x["tables"]) == BC.table_sets(y["tables"]), "a bucket holds other items"
        BC.assert_tables_well_formed(x["tables"])


def local_ids(O, v, p):
    """the local ids of pattern p decoded from the view's stream with the oracle's decoder: the first id is not coded, the last one is stored"""
    l, bits, last = int(v["num_local"][p]), int(v["num_bits"][p]), int(v["last_sample_id"][p])
    if l == 0:
        return []
    words = ((bits + 127) // 128) * 2 if bits else 0
    off = int(v["data_offset"][p])
    deltas = O.gamma_decode(v["data"][off: off + max(words, 2)], bits, max(l, 1)).astype(np.int64) if bits else np.zeros(0, np.int64)
    assert deltas.size == l - 1
    ids = last - (deltas.sum() - np.concatenate([[0], np.cumsum(deltas)]))
    return [int(x) for x in ids]


def finds_everything(O, path, lists):
    """OracleDB.one2all of every sample on the file == the counts from the lists themselves: every k-mer is found, with the right pattern"""
    odb = O.OracleDB(path)
    sets = [set(int(x) for x in q) for q in lists]
    for q in lists:
        want = [len(set(int(x) for x in q) & s) for s in sets]
        assert [int(x) for x in odb.one2all(np.asarray(q, np.uint64))] == want
    odb.close()


def first_item_offset(raw):
    """byte offset of the first stored (key, value) item of the file's tables (the value is the u32 at +4)"""
    x = BC.split_db(raw)
    pos = len(x["head"]) + 8
    for hdr, bv, items in x["tables"]:
        pos += 64 + len(bv)
        if hdr[1]:
            return pos
        pos += 8 * hdr[1]
    raise AssertionError("the file's tables are empty")


def pattern_header_offsets(raw):
    """byte offset of every 40-byte pattern header, by pattern id (num_kmers is the i64 at +0)"""
    x = BC.split_db(raw)
    base = len(x["head"]) + len(x["tables_raw"])
    pr = x["patterns_raw"]
    pos, out = 8, []
    while len(out) < x["P"]:
        (bs,) = struct.unpack_from("<Q", pr, pos)
        pos += 8
        end = pos + bs
        while pos < end:
            out.append(base + pos)
            (bits,) = struct.unpack_from("<I", pr, pos + 28)
            pos += BC.PAT_HEADER + ((bits + 127) // 128) * 16
    return out


def patched(raw, offset, fmt, change):
    """raw with the value of format `fmt` at `offset` replaced by change(value)"""
    out = bytearray(raw)
    (v,) = struct.unpack_from(fmt, out, offset)
    struct.pack_into(fmt, out, offset, change(v))
    return bytes(out)
