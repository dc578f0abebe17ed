#!/usr/bin/env python3
"""k_zstd_compress against k_snappy_compress on the SF1 write leg.

Every column of row group 0 (1,048,576 rows) of the lineitem-shaped SF1 table (pfloor/datagen.py, the generator
bench.py writes its input with) is encoded with pf_encode_chunk as the writer does (dictionary on, OPTIONAL without
nulls, default page size), once with SNAPPY and once with ZSTD, interleaved in one process on one context: WARMUP
unrecorded rounds, then ROUNDS recorded ones. Per column and in total: the compressor's kernel time (HIP events,
pf_encoded_chunk.snappy_ms: best and median), the bytes into and out of it for both codecs, what libzstd (pyarrow)
makes of the same page sections at levels 1 and 3 (each ZSTD page section of the chunk is first read back with
libzstd, so the probe also proves the frames), and the census of the forms chosen: blocks raw / RLE / compressed
and literals sections raw / RLE / Huffman (tree as direct or FSE-compressed weights). One JSON line per column
and one for the total.

    python tools/probe_zstd_write.py [--out profiles/zstd_write_sf1.json] [--rounds 20] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_write_hybrid import RG_ROWS, columns, stats   # noqa: E402  the same columns, the same summary

SNAPPY, ZSTD = 1, 6


def sections(out, field, tmp):
    """The compressed page sections (whole ZSTD frames) of an encoded chunk and their uncompressed sizes."""
    from pfloor import writer as W
    from pfloor.decoder import ParquetFile
    L = W.lib()
    name = field.name.encode()
    fields = (W.WriteField * 1)(W.WriteField(name, field.physical_type, 1, 0))
    w = C.c_void_p()
    path = os.path.join(tmp, "one.parquet")
    assert L.pf_writer_open(path.encode(), fields, 1, C.byref(w)) == 0
    assert L.pf_writer_add_chunk(w, 0, C.byref(out)) == 0
    assert L.pf_writer_end_row_group(w, RG_ROWS) == 0
    assert L.pf_writer_close(w) == 0
    with open(path, "rb") as f:
        data = f.read()
    res = []
    with ParquetFile(path) as pf:
        s, n = pf.chunk_range(0, 0)
        d = pf.chunk_desc(0, 0, 0)
        for i in range(d.n_pages):
            p = d.pages[i]
            lv = p.def_bytes + p.rep_bytes if p.page_type == 3 else 0
            assert p.is_compressed or p.page_type != 3
            res.append((data[s + p.offset + lv:s + p.offset + p.compressed_size], p.uncompressed_size - lv))
    return res


def block_census(frame, c):
    """Counts of block types and literals modes of one frame of this library's writer (RFC 8878 headers)."""
    d = frame[4]
    at = 5 + (1, 2, 4, 8)[d >> 6] if d >> 6 else 6
    while True:
        v = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
        at += 3
        last, bt, size = v & 1, (v >> 1) & 3, v >> 3
        c[("block_raw", "block_rle", "block_compressed")[bt]] += 1
        if bt == 2:
            b = frame[at:at + size]
            t = b[0] & 3
            c[("lit_raw", "lit_rle", "lit_huffman")[min(t, 2)]] += 1
            if t == 2:
                hdr = (3, 3, 4, 5)[(b[0] >> 2) & 3]
                c["weights_fse" if b[hdr] < 128 else "weights_direct"] += 1
        at += 1 if bt == 1 else size
        if last:
            return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zstd_write_sf1.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import pyarrow as pa
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder
    cols = columns()
    dec = GpuDecoder(0)
    dec.set_timing(True)
    enc = W.GpuColumnEncoder(dec)
    lines = []
    keys = ("block_raw", "block_rle", "block_compressed", "lit_raw", "lit_rle", "lit_huffman", "weights_direct", "weights_fse")
    total = {"column": "TOTAL", "snappy_ms_best": 0.0, "snappy_ms_median": 0.0, "zstd_ms_best": 0.0, "zstd_ms_median": 0.0,
             "in_bytes": 0, "snappy_bytes": 0, "zstd_bytes": 0, "libzstd1_bytes": 0, "libzstd3_bytes": 0, **{k: 0 for k in keys}}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name, (field, data, validity) in cols.items():
                ms = {SNAPPY: [], ZSTD: []}
                size = {}
                for r in range(args.warmup + args.rounds):
                    for codec in (SNAPPY, ZSTD):
                        o = enc.encode(field, data, validity, RG_ROWS, codec=codec)
                        if r >= args.warmup:
                            ms[codec].append(o.snappy_ms)
                        size[codec] = (o.snappy_in, o.snappy_out, o.data_encoding)
                census = {k: 0 for k in keys}
                lib1 = lib3 = 0
                for frame, usize in sections(o, field, tmp):   # o: the last ZSTD encode
                    raw = pa.Codec("zstd").decompress(frame, decompressed_size=usize, asbytes=True)
                    assert len(raw) == usize
                    lib1 += len(pa.Codec("zstd", 1).compress(raw, asbytes=True))
                    lib3 += len(pa.Codec("zstd", 3).compress(raw, asbytes=True))
                    block_census(frame, census)
                line = {"column": name, "physical_type": field.physical_type, "data_encoding": size[ZSTD][2], "rounds": args.rounds,
                        "snappy_ms": stats(ms[SNAPPY]), "zstd_ms": stats(ms[ZSTD]), "in_bytes": size[ZSTD][0],
                        "snappy_bytes": size[SNAPPY][1], "zstd_bytes": size[ZSTD][1], "libzstd1_bytes": lib1, "libzstd3_bytes": lib3,
                        **census}
                assert size[SNAPPY][0] == size[ZSTD][0]
                for k in ("in_bytes", "snappy_bytes", "zstd_bytes", "libzstd1_bytes", "libzstd3_bytes") + keys:
                    total[k] += line[k]
                for c, key in ((SNAPPY, "snappy"), (ZSTD, "zstd")):
                    total[key + "_ms_best"] += min(ms[c])
                    total[key + "_ms_median"] += float(np.median(ms[c]))
                lines.append(line)
                print(json.dumps(line), flush=True)
    finally:
        dec.close()
    total = {k: round(v, 4) if isinstance(v, float) else v for k, v in total.items()}
    lines.append(total)
    print(json.dumps(total), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
