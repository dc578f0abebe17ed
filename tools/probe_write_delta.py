#!/usr/bin/env python3
"""What the DELTA_* fallback costs and saves on the SF1 write leg.

Row group 0 (1,048,576 rows) of the lineitem-shaped SF1 table (pfloor/datagen.py, the generator
bench.py writes its input with) has four columns whose dictionary is over the 1 MiB page limit. Each
is encoded with pf_encode_chunk as the writer does (SNAPPY, dictionary on, default page size), with
PF_ENCODE_DELTA_FALLBACK clear (PLAIN fallback) and set (DELTA_BINARY_PACKED / DELTA_BYTE_ARRAY;
DOUBLE stays PLAIN), interleaved in one process: WARMUP unrecorded rounds, then ROUNDS recorded ones.
One JSON line per column: median / min / max of encode_ms and snappy_ms (HIP events), of the wall
time of the call (H2D of the column, kernels, D2H of the compressed pages, headers), and the chunk bytes.

    python tools/probe_write_delta.py [--out profiles/write_delta_sf1.json] [--rounds 9] [--warmup 3]
"""
import argparse
import json
import os
import sys
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


def stats(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_delta_sf1.json"))
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
        for name, (field, data, validity) in cols.items():
            first = enc.encode(field, data, validity, RG_ROWS)
            if first.fallback not in (1, 2):
                continue   # keeps its dictionary: the bit changes nothing
            rec = {False: [], True: []}
            info = {}
            for r in range(args.warmup + args.rounds):
                for delta in (False, True):
                    t0 = time.perf_counter()
                    o = enc.encode(field, data, validity, RG_ROWS, delta_fallback=delta)
                    wall = (time.perf_counter() - t0) * 1e3
                    info[delta] = {"data_encoding": o.data_encoding, "fallback": o.fallback, "chunk_bytes": o.size,
                                   "values_bytes": o.snappy_in, "pages": o.n_data_pages}
                    if r >= args.warmup:
                        rec[delta].append((o.encode_ms, o.snappy_ms, wall))
            line = {"column": name, "physical_type": field.physical_type, "rows": RG_ROWS, "rounds": args.rounds,
                    "warmup": args.warmup}
            for delta, key in ((False, "plain_fallback"), (True, "delta_fallback")):
                e, s, w = zip(*rec[delta])
                line[key] = dict(info[delta], encode_ms=stats(e), snappy_ms=stats(s), wall_ms=stats(w))
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
