#!/usr/bin/env python3
"""What the page index (PF_ENCODE_PAGE_INDEX) costs on the SF1 write leg.

Every column of row group 0 (1,048,576 rows) of the lineitem-shaped SF1 table (pfloor/datagen.py, the generator
bench.py writes its input with) is encoded with pf_encode_chunk as the writer does (SNAPPY, dictionary on,
OPTIONAL without nulls, default page size) with the bits clear, with statistics, with statistics and the index, and
with the index alone, interleaved in one process on one context: WARMUP unrecorded rounds, then ROUNDS recorded
ones. One JSON line per column: median / min / max of encode_ms (HIP events; the statistics kernels and k_enc_pgindex
are inside it) and of the wall time of the call, and one line with the sums over the columns per round.

    python tools/probe_write_pgindex.py [--out profiles/write_pgindex_sf1.json] [--rounds 20] [--warmup 3]

--default-only measures the default route alone and takes the package from --pkg (a checkout of another commit,
built): run alternately on two trees for an interleaved A/B of the route every caller has today.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = (("bits_clear", {}), ("statistics", dict(statistics=True)),
            ("statistics_page_index", dict(statistics=True, page_index=True)), ("page_index", dict(page_index=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "write_pgindex_sf1.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "parquet-floor_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from probe_write_hybrid import RG_ROWS, columns, stats   # the same columns, the same summary
    sys.path.insert(0, os.path.abspath(args.pkg))              # (in front of the tree probe_write_hybrid names)
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder
    settings = SETTINGS[:1] if args.default_only else SETTINGS
    cols = columns()
    dec = GpuDecoder(0)
    dec.set_timing(True)
    enc = W.GpuColumnEncoder(dec)
    lines = []
    total = {k: np.zeros(args.rounds) for k, _kw in settings}
    try:
        for name, (field, data, validity) in cols.items():
            rec = {k: [] for k, _kw in settings}
            info = {}
            for r in range(args.warmup + args.rounds):
                for key, kw in settings:
                    t0 = time.perf_counter()
                    o = enc.encode(field, data, validity, RG_ROWS, **kw)
                    wall = (time.perf_counter() - t0) * 1e3
                    if r >= args.warmup:
                        rec[key].append((o.encode_ms, o.snappy_ms, wall))
                        total[key][r - args.warmup] += o.encode_ms
                    info[key] = {"chunk_bytes": o.size, "pages": o.n_data_pages}
                    if "page_index" in kw:
                        info[key].update(column_index=o.column_index, boundary_order=o.boundary_order,
                                         index_value_bytes=int(o.index_value_off[2 * o.index_pages]) if o.column_index else 0)
            line = {"column": name, "physical_type": field.physical_type, "rows": RG_ROWS, "rounds": args.rounds, "warmup": args.warmup}
            for key, _kw in settings:
                e, s, w = zip(*rec[key])
                line[key] = dict(info[key], encode_ms=stats(e), snappy_ms=stats(s), wall_ms=stats(w))
            lines.append(line)
            print(json.dumps(line), flush=True)
    finally:
        dec.close()
    line = {"column": "*", "pkg": os.path.abspath(args.pkg), "encode_ms_sum": {k: stats(v) for k, v in total.items()}}
    lines.append(line)
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
