#!/usr/bin/env python3
"""What a row range costs and saves on the SF1 table.

Row group 0 (1,048,576 rows, 16 columns) of the lineitem-shaped SF1 table is written by the GPU writer with
page_index=True (default pages of 20,000 rows). A 100-row window around one l_orderkey value, found through
ParquetFile.candidate_rows, is read with plan_rows / decode(windows=...) / fetch across all 16 columns and compared
with a full decode plus fetch of the same row group on the same context: file bytes read, H2D bytes, D2H bytes, the
window kernels' time (HIP events) and the wall time of decode + wait + fetch (the file reads are timed apart). The
window is small, so its wall time measures overheads: launches, the per-array copies of fetch, Python.

    python tools/probe_row_window.py [--out profiles/row_window_sf1.json] [--reps 200] [--full-reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(xs):
    return round(float(np.median(xs)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_window_sf1.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--full-reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "parquet-floor_amd"))
    from probe_write_hybrid import RG_ROWS, columns
    from pfloor import writer as W
    from pfloor.decoder import GpuDecoder, ParquetFile
    cols = columns()
    names = list(cols)
    dec = GpuDecoder(0)
    dec.set_timing(True)
    out = {"rows": RG_ROWS, "columns": len(names), "reps": args.reps, "full_reps": args.full_reps, "warmup": args.warmup}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "sf1_rg0.parquet")
        w = W.ParquetWriter(W.MessageType("lineitem", *[cols[n][0] for n in names]), path, None, decoder=dec, page_index=True)
        w.write_columns({n: cols[n][1] for n in names}, RG_ROWS)
        w.close()
        out["file_bytes"] = os.path.getsize(path)
        with ParquetFile(path) as f:
            idx = list(range(f.num_columns))
            key_col = names.index("l_orderkey")
            row = RG_ROWS // 2 + 12345
            key = int(np.asarray(cols["l_orderkey"][1])[row])
            cand = f.candidate_rows(0, key_col, key, key)
            assert any(a <= row < b for a, b in cand), (cand, row)
            lo, hi = row - 50, row + 50
            out.update(key=key, candidate_rows=cand, window_rows=[lo, hi])
            types = [(f.columns[c].physical_type, f.columns[c].max_def, f.columns[c].max_rep) for c in idx]

            def d2h(arrs):
                return int(sum(v.nbytes for a in arrs for v in a.values() if isinstance(v, np.ndarray)))

            def full():
                t0 = time.perf_counter()
                items, total = f.plan([0], idx)
                buf = dec.staging(total)
                descs = []
                for _rg, col, s, n, off in items:
                    f.read_into(s, n, buf.ptr.value + off)
                    descs.append(f.chunk_desc(0, col, off))
                t1 = time.perf_counter()
                dec.decode(descs, buf.ptr.value, total)
                assert dec.wait() == 0, dec.error()
                arrs = [dec.fetch(i, *types[i]) for i in range(len(idx))]
                t2 = time.perf_counter()
                return arrs, sum(n for _rg, _c, _s, n, _o in items), total, (t1 - t0) * 1e3, (t2 - t1) * 1e3

            def window():
                t0 = time.perf_counter()
                items, total, wins = f.plan_rows(0, idx, lo, hi)
                buf = dec.staging(total)
                nread = f.read_rows(items, buf.ptr.value)
                t1 = time.perf_counter()
                dec.decode([d for _c, d, _r, _o in items], buf.ptr.value, max(total, 1), windows=wins)
                assert dec.wait() == 0, dec.error()
                arrs = [dec.fetch(i, *types[i]) for i in range(len(idx))]
                t2 = time.perf_counter()
                return arrs, nread, total, (t1 - t0) * 1e3, (t2 - t1) * 1e3, dec.window_ms()

            for label, fn, reps in (("full", full, args.full_reps), ("window", window, args.reps)):
                rec = []
                for r in range(args.warmup + reps):
                    res = fn()
                    if r >= args.warmup:
                        rec.append(res[3:])
                arrs, nread, h2d = res[0], res[1], res[2]
                line = {"file_bytes_read": int(nread), "h2d_bytes": int(h2d), "d2h_bytes": d2h(arrs),
                        "rows_returned": int(arrs[0]["num_rows"]), "read_ms": med([x[0] for x in rec]),
                        "decode_fetch_ms": med([x[1] for x in rec]),
                        "decode_fetch_ms_min_max": [round(min(x[1] for x in rec), 4), round(max(x[1] for x in rec), 4)]}
                if label == "window":
                    line["window_stage_ms"] = med([x[2] for x in rec])
                    # the rows are the written ones
                    got = np.frombuffer(arrs[key_col]["values"].tobytes(), np.int64)
                    assert np.array_equal(got, np.asarray(cols["l_orderkey"][1])[lo:hi]) and key in got
                out[label] = line
    dec.close()
    fl, wn = out["full"], out["window"]
    out["ratios_full_over_window"] = {k: round(fl[k] / max(wn[k], 1e-9), 1)
                                      for k in ("file_bytes_read", "h2d_bytes", "d2h_bytes", "decode_fetch_ms")}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        fo.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
