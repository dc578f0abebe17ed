#!/usr/bin/env python3
"""What statistics (PF_ENCODE_STATISTICS) and page CRCs (PF_ENCODE_PAGE_CRC) cost on the SF1 write leg.

Every column of row group 0 (1,048,576 rows) of the lineitem-shaped SF1 table (pfloor/datagen.py, the generator
bench.py writes its input with) is encoded with pf_encode_chunk as the writer does (SNAPPY, dictionary on,
OPTIONAL without nulls, default page size) with both bits clear, with bit 8 alone, with bit 16 alone and with
both, interleaved in one process on one context: WARMUP unrecorded rounds, then ROUNDS recorded ones. One JSON
line per column: median / min / max of encode_ms and snappy_ms (HIP events; the statistics and CRC kernels are
inside encode_ms) and of the wall time of the call, and the bytes the new kernels read: the dense values (strings:
their positions and lengths twice, and the characters of the first 8 bytes) and the stored page bytes.

    python tools/probe_write_stats.py [--out profiles/write_stats_sf1.json] [--rounds 9] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from probe_write_hybrid import RG_ROWS, columns, stats   # noqa: E402  the same columns, the same summary

SETTINGS = (("bits_clear", False, False), ("statistics", True, False), ("page_crc", False, True), ("both", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_stats_sf1.json"))
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
            rec = {k: [] for k, _s, _c in SETTINGS}
            info = {}
            for r in range(args.warmup + args.rounds):
                for key, st, crc in SETTINGS:
                    t0 = time.perf_counter()
                    o = enc.encode(field, data, validity, RG_ROWS, statistics=st, page_checksums=crc)
                    wall = (time.perf_counter() - t0) * 1e3
                    if r >= args.warmup:
                        rec[key].append((o.encode_ms, o.snappy_ms, wall))
                    info[key] = {"chunk_bytes": o.size, "data_encoding": o.data_encoding, "pages": o.n_data_pages,
                                 "stats_flags": o.stats_flags}
            if field.physical_type == 6:
                read = 2 * 8 * RG_ROWS + int(np.minimum(np.diff(data[0]), 8).sum()) * 2
            else:
                read = int(np.asarray(data).nbytes)
            line = {"column": name, "physical_type": field.physical_type, "rows": RG_ROWS, "rounds": args.rounds,
                    "warmup": args.warmup, "statistics_bytes_read": read, "crc_bytes_read": int(info["both"]["chunk_bytes"])}
            for key, _s, _c in SETTINGS:
                e, s, w = zip(*rec[key])
                line[key] = dict(info[key], encode_ms=stats(e), snappy_ms=stats(s), wall_ms=stats(w))
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
