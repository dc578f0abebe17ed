#!/usr/bin/env python3
"""What parquet-mr's hybrid runs (PF_ENCODE_HYBRID_RUNS) cost and save on the SF1 write leg.

Every column of row group 0 (1,048,576 rows) of the lineitem-shaped SF1 table (pfloor/datagen.py, the
generator bench.py writes its input with) is encoded with pf_encode_chunk as the writer does (SNAPPY,
dictionary on, OPTIONAL without nulls, default page size), with the bit clear (ids and levels one
bit-packed run per page) and set (RLE runs and bit-packed groups, encoded on the GPU), interleaved in
one process on one context: WARMUP unrecorded rounds, then ROUNDS recorded ones. One JSON line per
column: chunk bytes, the bytes of its definition levels, and median / min / max of encode_ms and
snappy_ms (HIP events) and of the wall time of the call (H2D of the column, kernels, D2H of the pages,
headers).

    python tools/probe_write_hybrid.py [--out profiles/write_hybrid_sf1.json] [--rounds 9] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))

SF1_ROWS, RG_ROWS, SEED = 6001215, 1 << 20, 42   # bench.py's sf1 workload
PTYPE = {"int32": 1, "int64": 2, "float": 4, "double": 5, "string": 6, "large_string": 6}


def columns():
    """{name: (Field, data, validity)} of row group 0, as bench.py's write leg passes them."""
    from pfloor import datagen
    from pfloor import writer as W
    t = datagen.lineitem_table(SF1_ROWS, seed=SEED).slice(0, RG_ROWS)
    validity = np.packbits(np.ones(RG_ROWS, bool), bitorder="little")
    out = {}
    for name in t.column_names:
        a = t.column(name).combine_chunks()
        pt = PTYPE[str(a.type)]
        if pt == 6:
            offs = np.frombuffer(a.buffers()[1], np.int32, RG_ROWS + 1, a.offset * 4)
            chars = np.frombuffer(a.buffers()[2], np.uint8)[offs[0]:offs[-1]]
            data = ((offs - offs[0]).astype(np.int32), chars)
        else:
            data = a.to_numpy(zero_copy_only=False)
        out[name] = (W.Field(name, pt, True, pt == 6), data, validity)
    return out


def level_bytes(out, field, tmp):
    """Bytes of the definition levels of an encoded chunk: the def_bytes of its v2 page headers."""
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
    with ParquetFile(path) as pf:
        d = pf.chunk_desc(0, 0, 0)
        return int(sum(d.pages[i].def_bytes for i in range(d.n_pages) if d.pages[i].page_type == 3))


def stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_hybrid_sf1.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder
    cols = columns()
    dec = GpuDecoder(0)
    dec.set_timing(True)
    enc = W.GpuColumnEncoder(dec)
    lines = []
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for name, (field, data, validity) in cols.items():
                rec = {False: [], True: []}
                info = {}
                for hyb in (False, True):
                    o = enc.encode(field, data, validity, RG_ROWS, hybrid_runs=hyb)
                    info[hyb] = {"data_encoding": o.data_encoding, "fallback": o.fallback, "dict_entries": o.dict_entries,
                                 "chunk_bytes": o.size, "values_bytes": o.snappy_in, "pages": o.n_data_pages}
                    info[hyb]["level_bytes"] = level_bytes(o, field, tmp)
                for r in range(args.warmup + args.rounds):
                    for hyb in (False, True):
                        t0 = time.perf_counter()
                        o = enc.encode(field, data, validity, RG_ROWS, hybrid_runs=hyb)
                        wall = (time.perf_counter() - t0) * 1e3
                        if r >= args.warmup:
                            rec[hyb].append((o.encode_ms, o.snappy_ms, wall))
                line = {"column": name, "physical_type": field.physical_type, "rows": RG_ROWS, "rounds": args.rounds,
                        "warmup": args.warmup}
                for hyb, key in ((False, "bit_clear"), (True, "hybrid_runs")):
                    e, s, w = zip(*rec[hyb])
                    line[key] = dict(info[hyb], encode_ms=stats(e), snappy_ms=stats(s), wall_ms=stats(w))
                lines.append(line)
                print(json.dumps(line), flush=True)
    finally:
        dec.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
