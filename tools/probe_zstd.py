"""ZSTD against Snappy on one SF1 row group: the first 1 Mi rows of the lineitem table (seed 42, all 16
columns) written by pyarrow at zstd level 3 and in Snappy, chunk bytes resident on the device, decoded
REPS times with HIP-event stage times. Prints, per codec, file bytes, decoded GB/s (best and median)
and the stage times of the best run; for ZSTD the decompression stage is k_zstd alone.

  python tools/probe_zstd.py [REPS]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "parquet-floor_amd")]
import numpy as np  # noqa: E402
import pyarrow.parquet as pq  # noqa: E402
from pfloor import _native, datagen  # noqa: E402
from pfloor.decoder import GpuDecoder, ParquetFile  # noqa: E402

ROWS = 1 << 20
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_dir = os.environ.get("PF_BENCH_DIR", "/tmp/pfloor_bench")
os.makedirs(out_dir, exist_ok=True)
table = None
result = {}
for codec, kw in (("snappy", dict(compression="snappy")), ("zstd", dict(compression="zstd", compression_level=3))):
    path = os.path.join(out_dir, f"probe_zstd_lineitem_{ROWS}_{codec}.parquet")
    if not os.path.exists(path):
        table = table if table is not None else datagen.lineitem_table(ROWS, seed=42)
        pq.write_table(table, path, row_group_size=ROWS, **kw)
    L = _native.lib()
    with ParquetFile(path) as pf, GpuDecoder(0) as dec:
        items, total = pf.plan([0], list(range(pf.num_columns)))
        host = np.zeros(max(total, 1), np.uint8)
        descs = []
        for rg, col, s, n, off in items:
            pf.read_into(s, n, host.ctypes.data + off)
            descs.append(pf.chunk_desc(rg, col, off))
        dptr = C.c_void_p()
        _native.check(L.pf_device_alloc(dec.h, total, C.byref(dptr)), dec.h, "pf_device_alloc")
        _native.check(L.pf_memcpy_h2d(dec.h, dptr, host.ctypes.data, total), dec.h, "pf_memcpy_h2d")
        dec.set_timing(True)
        runs = []
        for _ in range(reps + 2):
            dec.decode(descs, dptr.value, total, on_device=True)
            rc = dec.wait()
            assert rc == 0, dec.error()
            runs.append(dec.timing())
        runs = runs[2:]   # warm-up: arena growth
        decoded = 0
        for i, (rg, col, *_r) in enumerate(items):
            ci = dec.info(i)
            decoded += ci.num_slots * ci.width + ci.num_chars + (4 * (ci.num_slots + 1) if pf.columns[col].physical_type == 6 else 0)
        totals = [sum(r.values()) for r in runs]
        best = runs[totals.index(min(totals))]
        result[codec] = dict(file_bytes=os.path.getsize(path), chunk_bytes=total, decoded_bytes=int(decoded),
                             best_ms=min(totals), median_ms=statistics.median(totals),
                             best_gbs=decoded / min(totals) / 1e6, median_gbs=decoded / statistics.median(totals) / 1e6,
                             decompress_ms_best=best["snappy_parse"] + best["snappy_exec"],
                             decompress_ms_median=statistics.median(r["snappy_parse"] + r["snappy_exec"] for r in runs),
                             stages_best={k: round(v, 4) for k, v in best.items()})
        L.pf_device_free(dec.h, dptr)
print(json.dumps(result))
